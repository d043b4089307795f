// libliinit_hip — KD_TREE::Nearest_Search for arbitrary points, k and max_dist (lii_map_nearest / lii_map_nearest_dev).
// Reference: include/ikd-Tree/ikd_Tree.cpp:349-379 (Nearest_Search), :825-968 (Search), :1273-1277 (calc_dist).
// A unit of its own on top of the grid's addressing (lii_grid.h): the searches of the registration pass (lii_knn.hip, lii_fit.hip) are
// specialised for five neighbours inside 3 x 3 x 3 blocks of cells and are not touched.
//
// ONE WAVEFRONT PER QUERY.  The result list is the wavefront itself: lane j holds entry j - (d2, slot in the point array) - and the
// 64 lanes are kept ascending in d2 (free entries: +inf), so the k-th distance is lane k - 1 for every k <= 64.  The cells around the
// query's cell are visited in Chebyshev rings r = 0, 1, 2, ...: every lane takes one cell of the ring and looks its [first, end) up,
// a wave-wide prefix sum lays the ranges of the 64 cells end to end, and the wavefront walks that sequence 64 points at a time (a
// lane finds the cell of its point by a binary search over the prefix, six lane reads).  A candidate is a point with d2 <= max_dist
// and d2 < the k-th distance; the candidates of a batch enter one by one in lane order: position = popcount of a ballot, shift = a
// lane shift.  An equal d2 goes BEHIND the entries already held, and a candidate equal to the k-th distance of a full list stays out.
// After ring r the search ends when the list is full and its k-th distance lies inside the visited cube, or when the cube covers
// the ball of radius sqrt(max_dist); ring r_max = ceil(sqrt(max_dist) / cell) + 1 always does.
// Every loop is bounded by a number known before it starts: rings (r_max <= 34), cells of a ring, points of 64 cells, 64 candidates,
// slots of the block table.  No workgroup waits for anything.
// The ball query (lii_map_radius / lii_map_radius_dev: every point within max_dist) stands behind it in this file, on the same walk.
// (the walk itself - ring_walk_nearest - and what it stands on live in lii_ringwalk.h: the pose scoring, lii_score.hip, searches by it too)
#include "lii_launch.h"
#include "lii_ringwalk.h"

namespace lii {
namespace {

constexpr int kQueryWaves = kBlock / 64;  // queries per workgroup

// W: floats a row of pts_out - 3, or 4 with the stored fourth word (the point's intensity) behind x, y, z; one more load per row written
template <int W>
__global__ __launch_bounds__(kBlock) void k_map_nearest(GridView g, unsigned int n_entries, unsigned int pts_cap, const char* __restrict__ queries,
                                                        int n, int stride_bytes, int k, float max_d2, int r_max, float* __restrict__ pts_out,
                                                        float* __restrict__ d2_out, int* __restrict__ count_out) {
  const int lane = threadIdx.x & 63;
  const long long qi = (long long)blockIdx.x * kQueryWaves + (threadIdx.x >> 6);
  if (qi >= n) return;  // (the whole wavefront)
  const float* qp = reinterpret_cast<const float*>(queries + (size_t)qi * (size_t)stride_bytes);
  const float qx = qp[0], qy = qp[1], qz = qp[2];
  float my_d;
  unsigned int my_i;
  ring_walk_nearest(g, n_entries, pts_cap, qx, qy, qz, k, max_d2, r_max, my_d, my_i);
  const int count = __popcll(__ballot(lane < k && my_i != kFree));
  if (lane == 0) count_out[qi] = count;
  if (lane < k) {
    float ox = 0.f, oy = 0.f, oz = 0.f, ow = 0.f, od = 0.f;
    if (lane < count) {
      const F3 m = load_xyz(g.pts, my_i);
      ox = m.x; oy = m.y; oz = m.z; od = my_d;
      if (W == 4) ow = g.pts[my_i].w;
    }
    const size_t row = (size_t)qi * (size_t)k + (size_t)lane;
    if (pts_out) {
      pts_out[W * row] = ox; pts_out[W * row + 1] = oy; pts_out[W * row + 2] = oz;
      if (W == 4) pts_out[W * row + 3] = ow;
    }
    if (d2_out) d2_out[row] = od;
  }
}

}  // namespace

void launch_map_nearest(const GridView& g, unsigned int n_entries, unsigned int pts_cap, const void* queries, int n, int stride_bytes, int k,
                        float max_d2, int r_max, float* pts_out, float* d2_out, int* count_out, hipStream_t s, int row_floats) {
  if (n <= 0) return;
  const unsigned int blocks = (unsigned int)(((long long)n + kQueryWaves - 1) / kQueryWaves);
  if (row_floats == 4)
    hipLaunchKernelGGL(k_map_nearest<4>, dim3(blocks), dim3(kBlock), 0, s, g, n_entries, pts_cap, static_cast<const char*>(queries), n, stride_bytes, k,
                       max_d2, r_max, pts_out, d2_out, count_out);
  else
    hipLaunchKernelGGL(k_map_nearest<3>, dim3(blocks), dim3(kBlock), 0, s, g, n_entries, pts_cap, static_cast<const char*>(queries), n, stride_bytes, k,
                       max_d2, r_max, pts_out, d2_out, count_out);
}

// ------------------------------------------------------------------------------------------------ the ball query
// KD_TREE::Radius_Search of upstream ikd-Tree - in the reference's copy of the tree Nearest_Search(point, k, ..., max_dist) with k above
// the ball's population - (lii_map_radius / lii_map_radius_dev): EVERY live point with d2 <= max_dist, however many there are.
// ONE WAVEFRONT PER QUERY, and a query walks its cells TWICE, by ball_walk (lii_ringwalk.h; the surface statistics of lii_surface.hip
// reduce a ball on the same walk): Chebyshev rings, one cell per lane, cell_range_checked, the per-cell gap bound against max_d2 alone,
// the wave-wide prefix over 64 cells, 64 points at a time.  The count
// pass leaves the sum of the ballots' popcounts; an exclusive scan of the counts (lii_sort.hip) makes them offsets; the fill pass
// repeats the identical walk and stores an accepted point at offsets[i] + (points accepted so far) + (popcount of the ballot below the
// lane): the segments are dense and in the walk's order, and no atomic touches the output.  There is no k-th distance to stop on: ring
// r_max is always reached.  Every loop is bounded by a number known before it starts; no workgroup waits for anything.
// What the fill pass may write is bounded twice: by the segment [offsets[i], offsets[i + 1]) - a walk that met more points than the
// count pass did (it cannot: both launches sit behind every map update on the stream) stores none of them - and by `capacity` rows.
namespace {

template <bool kFill, int W>
__global__ __launch_bounds__(kBlock) void k_map_radius(GridView g, unsigned int n_entries, unsigned int pts_cap, const char* __restrict__ queries, int n,
                                                       int stride_bytes, float max_d2, int r_max, long long* __restrict__ count_out,
                                                       const long long* __restrict__ offsets, long long base, long long capacity,
                                                       float* __restrict__ pts_out, float* __restrict__ d2_out,
                                                       unsigned long long* __restrict__ key_out, unsigned int* __restrict__ slot_out) {
  const int lane = threadIdx.x & 63;
  const long long qi = (long long)blockIdx.x * kQueryWaves + (threadIdx.x >> 6);
  if (qi >= n) return;  // (the whole wavefront)
  const float* qp = reinterpret_cast<const float*>(queries + (size_t)qi * (size_t)stride_bytes);
  const float qx = qp[0], qy = qp[1], qz = qp[2];
  // (a NaN coordinate: an empty segment; a ball that reaches no addressable cell: one as well - ball_walk makes no trip then)
  bool wanted = true;
  long long seg_first = 0;
  unsigned int seg_len = 0u;
  if (kFill) {
    const long long o0 = offsets[qi], o1 = offsets[qi + 1];
    seg_first = o0 - base;
    seg_len = (unsigned int)min(max(o1 - o0, 0ll), (long long)pts_cap);  // (a ball holds no more points than the array has slots)
    wanted = seg_len > 0u && seg_first >= 0 && seg_first < capacity;  // (an empty segment, or one beyond the rows: no walk)
  }
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned int accepted = 0u;
  ball_walk(g, n_entries, pts_cap, qx, qy, qz, max_d2, r_max, wanted,
            [&](unsigned int slot, bool, bool in_ball, unsigned long long hits, float mx, float my, float mz, float d) {
              if (kFill) {
                const unsigned int at = accepted + (unsigned int)__popcll(hits & below);
                const long long row = seg_first + (long long)at;
                if (in_ball && at < seg_len && row < capacity) {
                  if (pts_out) {
                    pts_out[W * row] = mx; pts_out[W * row + 1] = my; pts_out[W * row + 2] = mz;
                    if (W == 4) pts_out[W * row + 3] = g.pts[slot].w;
                  }
                  if (d2_out) d2_out[row] = d;
                  if (key_out) key_out[row] = ((unsigned long long)qi << 32) | (unsigned long long)__float_as_uint(d);
                  if (slot_out) slot_out[row] = slot;
                }
              }
              accepted += (unsigned int)__popcll(hits);
            });
  if (!kFill && lane == 0) count_out[qi] = (long long)accepted;
}

// LII_RADIUS_SORTED, behind the sort of (query << 32 | d2 bits, slot): row r of the result is the point in slot slots[r] at the d2 in the
// key's low word.  rows = min(total[0] - base, capacity) is read from the device (the device form does not know the total on the host).
template <int W>
__global__ __launch_bounds__(kBlock) void k_radius_gather(const float4* __restrict__ pts, unsigned int pts_cap, const unsigned long long* __restrict__ keys,
                                                          const unsigned int* __restrict__ slots, const long long* __restrict__ total, long long base,
                                                          long long capacity, float* __restrict__ pts_out, float* __restrict__ d2_out) {
  const long long rows = min(max(total[0] - base, 0ll), capacity);
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long row = (long long)blockIdx.x * kBlock + threadIdx.x; row < rows; row += stride) {  // (rows is fixed before the loop starts)
    if (d2_out) d2_out[row] = __uint_as_float((unsigned int)(keys[row] & 0xFFFFFFFFull));
    if (pts_out) {
      const unsigned int slot = slots[row];
      float x = 0.f, y = 0.f, z = 0.f, w = 0.f;
      if (slot < pts_cap) {
        const F3 m = load_xyz(pts, slot);
        x = m.x; y = m.y; z = m.z;
        if (W == 4) w = pts[slot].w;
      }
      pts_out[W * row] = x; pts_out[W * row + 1] = y; pts_out[W * row + 2] = z;
      if (W == 4) pts_out[W * row + 3] = w;
    }
  }
}

}  // namespace

void launch_map_radius_count(const GridView& g, unsigned int n_entries, unsigned int pts_cap, const void* queries, int n, int stride_bytes, float max_d2,
                             int r_max, long long* count_out, hipStream_t s) {
  if (n <= 0) return;
  const unsigned int blocks = (unsigned int)(((long long)n + kQueryWaves - 1) / kQueryWaves);
  hipLaunchKernelGGL((k_map_radius<false, 3>), dim3(blocks), dim3(kBlock), 0, s, g, n_entries, pts_cap, static_cast<const char*>(queries), n, stride_bytes,
                     max_d2, r_max, count_out, (const long long*)nullptr, 0ll, 0ll, (float*)nullptr, (float*)nullptr, (unsigned long long*)nullptr,
                     (unsigned int*)nullptr);
}

void launch_map_radius_fill(const GridView& g, unsigned int n_entries, unsigned int pts_cap, const void* queries, int n, int stride_bytes, float max_d2,
                            int r_max, const long long* offsets, long long base, long long capacity, float* pts_out, float* d2_out,
                            unsigned long long* key_out, unsigned int* slot_out, hipStream_t s, int row_floats) {
  if (n <= 0 || capacity <= 0) return;
  const unsigned int blocks = (unsigned int)(((long long)n + kQueryWaves - 1) / kQueryWaves);
  if (row_floats == 4)
    hipLaunchKernelGGL((k_map_radius<true, 4>), dim3(blocks), dim3(kBlock), 0, s, g, n_entries, pts_cap, static_cast<const char*>(queries), n, stride_bytes,
                       max_d2, r_max, (long long*)nullptr, offsets, base, capacity, pts_out, d2_out, key_out, slot_out);
  else
    hipLaunchKernelGGL((k_map_radius<true, 3>), dim3(blocks), dim3(kBlock), 0, s, g, n_entries, pts_cap, static_cast<const char*>(queries), n, stride_bytes,
                       max_d2, r_max, (long long*)nullptr, offsets, base, capacity, pts_out, d2_out, key_out, slot_out);
}

void launch_map_radius_gather(const GridView& g, unsigned int pts_cap, const unsigned long long* keys, const unsigned int* slots, const long long* total,
                              long long base, long long capacity, float* pts_out, float* d2_out, hipStream_t s, int row_floats) {
  if (capacity <= 0) return;
  const long long want = (capacity - 1) / kBlock + 1;
  const unsigned int blocks = want < 2048 ? (unsigned int)want : 2048u;  // (grid-stride beyond that)
  if (row_floats == 4) hipLaunchKernelGGL(k_radius_gather<4>, dim3(blocks), dim3(kBlock), 0, s, g.pts, pts_cap, keys, slots, total, base, capacity, pts_out, d2_out);
  else hipLaunchKernelGGL(k_radius_gather<3>, dim3(blocks), dim3(kBlock), 0, s, g.pts, pts_cap, keys, slots, total, base, capacity, pts_out, d2_out);
}

}  // namespace lii
