// What the search launch (lii_knn.hip) and the fit / completion launch (lii_fit.hip) share beyond the grid's addressing (lii_grid.h).
#pragma once
#include "lii_grid.h"

namespace lii {

__device__ __forceinline__ float axis_gap(float q, int c, float cs, float eps) {
  float lo = (float)c * cs - eps, hi = (float)(c + 1) * cs + eps;
  return fmaxf(fmaxf(lo - q, q - hi), 0.f);
}

// blocks are remapped so that each XCD (block b runs on XCD b % 8) works on a CONTIGUOUS eighth of the point
// stream: neighbouring scan points touch the same map cells, which then stay in that XCD's private 4 MiB L2
__device__ __forceinline__ int xcd_remap(int b, int nb_real) {
  const int per = (nb_real + 7) >> 3;  // the grid is launched with 8 * per blocks
  return (b & 7) * per + (b >> 3);
}

struct F3 {
  float x, y, z;
};
// xyz of map slot `idx`: 12 of the 16 bytes (w is the point's intensity).  The byte offset is formed in 32 bits (the point array holds
// fewer than 2^28 slots), so the load takes the uniform base from scalar registers and ONE address register.
__device__ __forceinline__ F3 load_xyz(const float4* __restrict__ pts, unsigned int idx) {
  typedef float f3v __attribute__((ext_vector_type(3)));
  const f3v v = *reinterpret_cast<const f3v*>(reinterpret_cast<const char*>(pts) + (size_t)(idx << 4));
  F3 r;
  r.x = v.x; r.y = v.y; r.z = v.z;
  return r;
}

// upper bound of the points one rank registers (the exact split is taken on the device from the exact cloud size)
static inline int shard_bound(const RegistrationBuffers& rb) {
  return rb.shard_world > 1 ? (rb.n + rb.shard_world - 1) / rb.shard_world + 1 : rb.n;
}

}  // namespace lii
