// The map index of the LI-Init hot path for gfx950 (CDNA4, wave64): its construction from a point set.  Hand-written.
//
// Kernels and the reference code they replace (paths relative to the reference root):
//   k_map_keys / k_map_gather / k_block_flags / k_cells_fill / k_win_bbox / k_win_fill
//                      device mirror of the ikd-Tree point set as a cell-sorted array + block-hierarchical grid, and the dense cell
//                      window over the map's box (include/ikd-Tree/ikd_Tree.cpp:336-347 Build)
//   k_body_to_map      the first scan seeds the map (src/laserMapping.cpp:921-929)
//   (searching the index: lii_knn.hip, lii_fit.hip; updating it in place: lii_map.hip)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "lii_grid.h"
#include "lii_launch.h"

namespace lii {

// ------------------------------------------------------------------------------------------------
// map index construction
__global__ void k_map_keys(const float4* __restrict__ pts, int n, float inv_cs, unsigned long long* __restrict__ keys,
                           unsigned int* __restrict__ idx) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float4 p = pts[i];
  keys[i] = point_key(cell_of(p.x, inv_cs), cell_of(p.y, inv_cs), cell_of(p.z, inv_cs));
  idx[i] = (unsigned)i;
}

__global__ void k_map_gather(const float4* __restrict__ src, const unsigned int* __restrict__ idx, int n,
                             float4* __restrict__ dst) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  dst[i] = src[idx[i]];
}

// flags[i] = 1 where a new 8x8x8 block starts in the sorted key array (inclusive scan of it = block id + 1)
__global__ void k_block_flags(const unsigned long long* __restrict__ keys, int n, unsigned int* __restrict__ flags) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  flags[i] = (i == 0 || (keys[i] >> 9) != (keys[i - 1] >> 9)) ? 1u : 0u;
}

__global__ void k_table_clear(BlockEntry* blocks, unsigned int cap) {
  unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cap) {
    BlockEntry e;
    e.key = kEmptyKey;
    e.id = 0;
    e.pad = 0;
    blocks[i] = e;
  }
}

// cells must be zero-filled for the n_blocks * 512 entries in use
__global__ void k_cells_fill(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ ranks, int n,
                             BlockEntry* blocks, unsigned int block_mask, uint2* __restrict__ cells, unsigned long long* __restrict__ key_of_id) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long key = keys[i];
  const bool is_start = (i == 0) || (keys[i - 1] != key);
  const bool is_end = (i == n - 1) || (keys[i + 1] != key);
  if (!is_start && !is_end) return;
  const unsigned int id = ranks[i] - 1;
  const unsigned int local = (unsigned int)(key & 511u);
  unsigned int* cell = reinterpret_cast<unsigned int*>(&cells[(size_t)id * kBlockCells + local]);
  if (is_start) cell[0] = (unsigned)i;
  if (is_end) cell[1] = (unsigned)(i + 1);
  if (is_start && ((i == 0) || ((keys[i - 1] >> 9) != (key >> 9)))) {
    const unsigned long long bk = key >> 9;
    if (key_of_id) key_of_id[id] = bk;  // (WinKeep: the block's coordinates by its id)
    unsigned int bx, by, bz;
    unpack_block(bk, bx, by, bz);
    unsigned int slot = hash_block((int)bx, (int)by, (int)bz) & block_mask;
    while (true) {
      unsigned long long prev = atomicCAS(&blocks[slot].key, kEmptyKey, bk);
      if (prev == kEmptyKey) { blocks[slot].id = id; blocks[slot].pad = 1u; break; }  // pad = "id is valid" (k_ins_cells waits on it)
      slot = (slot + 1) & block_mask;
    }
  }
}

// (body_to_world - pointBodyToWorld - lives in lii_device.h: lii_publish.hip uses it as well)
// The first scan seeds the map (src/laserMapping.cpp:921-929): the down-sampled cloud in the world frame, as map points (w = 0)
__global__ __launch_bounds__(256) void k_body_to_map(const float4* __restrict__ body, int n, PoseArg ps, float4* __restrict__ dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float wx, wy, wz;
  body_to_world(ps, body[i], wx, wy, wz);
  dst[i] = make_float4(wx, wy, wz, 0.f);
}
// ... with the cloud's intensities as the map points' fourth word (lii_map_intensity_set; pointBodyToWorld copies it, src/laserMapping.cpp:219)
__global__ __launch_bounds__(256) void k_body_to_map_w(const float4* __restrict__ body, const float* __restrict__ inten, int n, PoseArg ps, float4* __restrict__ dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float wx, wy, wz;
  body_to_world(ps, body[i], wx, wy, wz);
  dst[i] = make_float4(wx, wy, wz, inten[i]);
}

// ---- dense cell window (GridView::win) ---------------------------------------------------------------------------------------------
// box[0..2] = min, box[3..5] = max of the BIASED block coordinates over the occupied slots of the block table
__global__ void k_win_bbox(const BlockEntry* __restrict__ blocks, unsigned int cap, unsigned int* __restrict__ box) {
  const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cap) return;
  const unsigned long long k = blocks[i].key;
  if (k == kEmptyKey) return;
  unsigned int bx, by, bz;
  unpack_block(k, bx, by, bz);
  atomicMin(&box[0], bx); atomicMin(&box[1], by); atomicMin(&box[2], bz);
  atomicMax(&box[3], bx); atomicMax(&box[4], by); atomicMax(&box[5], bz);
}
// one workgroup of 512 lanes per slot of the block table: the 512 cell entries of an occupied block go to their places in the window
__global__ __launch_bounds__(512) void k_win_fill(const BlockEntry* __restrict__ blocks, const uint2* __restrict__ cells, uint2* __restrict__ win,
                                                  int wx0, int wy0, int wz0, int wnx, int wny, int wnz) {
  const BlockEntry e = blocks[blockIdx.x];
  if (e.key == kEmptyKey) return;
  const int bb = kCellBias >> kCoarseShift;
  unsigned int kx, ky, kz;
  unpack_block(e.key, kx, ky, kz);
  const int bx = (int)kx - bb, by = (int)ky - bb, bz = (int)kz - bb;
  const int l = threadIdx.x;
  const unsigned int ux = (unsigned)(bx * 8 + (l & 7) - wx0), uy = (unsigned)(by * 8 + ((l >> 3) & 7) - wy0), uz = (unsigned)(bz * 8 + (l >> 6) - wz0);
  if (ux < (unsigned)wnx && uy < (unsigned)wny && uz < (unsigned)wnz) win[((size_t)uz * wny + uy) * wnx + ux] = cells[(size_t)e.id * kBlockCells + l];
}

// ------------------------------------------------------------------------------------------------
// launchers
static inline int nblk(int n, int b) { return (n + b - 1) / b; }

void launch_map_keys(const float4* pts, int n, float inv_cs, unsigned long long* keys, unsigned int* idx, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_map_keys, dim3(nblk(n, 256)), dim3(256), 0, s, pts, n, inv_cs, keys, idx);
}
void launch_body_to_map(const float4* body, int n, const PoseArg& ps, float4* dst, hipStream_t s, const float* inten) {
  if (n > 0 && inten) {
    hipLaunchKernelGGL(k_body_to_map_w, dim3((n + 255) / 256), dim3(256), 0, s, body, inten, n, ps, dst);
    return;
  }
  if (n <= 0) return;
  hipLaunchKernelGGL(k_body_to_map, dim3(nblk(n, 256)), dim3(256), 0, s, body, n, ps, dst);
}
void launch_map_gather(const float4* src, const unsigned int* idx, int n, float4* dst, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_map_gather, dim3(nblk(n, 256)), dim3(256), 0, s, src, idx, n, dst);
}
void launch_block_flags(const unsigned long long* keys, int n, unsigned int* flags, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_block_flags, dim3(nblk(n, 256)), dim3(256), 0, s, keys, n, flags);
}
void launch_win_bbox(const BlockEntry* blocks, unsigned int cap, unsigned int* box, hipStream_t s) {
  hipLaunchKernelGGL(k_win_bbox, dim3((cap + 255) / 256), dim3(256), 0, s, blocks, cap, box);
}
void launch_win_fill(const BlockEntry* blocks, unsigned int cap, const uint2* cells, uint2* win, const int org[3], const int dim[3], hipStream_t s) {
  hipLaunchKernelGGL(k_win_fill, dim3(cap), dim3(512), 0, s, blocks, cells, win, org[0], org[1], org[2], dim[0], dim[1], dim[2]);
}
void launch_table_clear(BlockEntry* blocks, unsigned int cap, hipStream_t s) {
  hipLaunchKernelGGL(k_table_clear, dim3(nblk((int)cap, 256)), dim3(256), 0, s, blocks, cap);
}
void launch_cells_fill(const unsigned long long* keys, const unsigned int* ranks, int n, BlockEntry* blocks,
                       unsigned int block_mask, uint2* cells, unsigned long long* key_of_id, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_cells_fill, dim3(nblk(n, 256)), dim3(256), 0, s, keys, ranks, n, blocks, block_mask, cells, key_of_id);
}
}  // namespace lii
