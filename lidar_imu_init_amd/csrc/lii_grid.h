// The map grid's addressing, once: how a point finds its 8 x 8 x 8 block (key, hash, table probe) and its cell inside the block, and the
// float32 distance the searches rank by.  Shared by the units that build the index (lii_mapindex.hip), search it (lii_knn.hip,
// lii_fit.hip) and update it in place (lii_map.hip); the tables themselves - BlockEntry, GridView - are in lii_device.h.
#pragma once
#include "lii_device.h"

namespace lii {

constexpr int kBlockCells = 512;  // 8 x 8 x 8 cells per block

// sort key of a map point: (Bz, By, Bx) block key in the high bits, local cell (lz, ly, lx) in the low 9
__device__ __forceinline__ unsigned long long pack_block(int bx, int by, int bz) {  // biased block coordinates
  return ((unsigned long long)(unsigned)bz << 36) | ((unsigned long long)(unsigned)by << 18) | (unsigned long long)(unsigned)bx;
}
// ... and back: the biased block coordinates of a block key (18 bits each)
__device__ __forceinline__ void unpack_block(unsigned long long bk, unsigned int& bx, unsigned int& by, unsigned int& bz) {
  bx = (unsigned)(bk & 0x3FFFF); by = (unsigned)((bk >> 18) & 0x3FFFF); bz = (unsigned)((bk >> 36) & 0x3FFFF);
}
// index of cell (ix, iy, iz) among the 512 of its block, x fastest (biased or not: the bias is a multiple of eight)
__device__ __forceinline__ unsigned int local_cell(int ix, int iy, int iz) {
  return (((unsigned)iz & 7u) << 6) | (((unsigned)iy & 7u) << 3) | ((unsigned)ix & 7u);
}
__device__ __forceinline__ unsigned long long point_key(int cx, int cy, int cz) {
  const unsigned ux = (unsigned)(cx + kCellBias), uy = (unsigned)(cy + kCellBias), uz = (unsigned)(cz + kCellBias);
  const unsigned long long bk = pack_block((int)(ux >> kCoarseShift), (int)(uy >> kCoarseShift), (int)(uz >> kCoarseShift));
  const unsigned local = local_cell((int)ux, (int)uy, (int)uz);
  return (bk << 9) | local;
}
__device__ __forceinline__ unsigned int hash_key(unsigned long long k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return (unsigned int)k;
}
__device__ __forceinline__ unsigned int hash_block(int bx, int by, int bz) {
  // block coordinates are < 2^18 after biasing: 24-bit multiplies are full-rate VALU ops
  return (__umul24((unsigned)bx, 7919u * 1021u) ^ __umul24((unsigned)by, 104729u * 13u) ^ __umul24((unsigned)bz, 1299709u)) * 2654435761u;
}

__device__ __forceinline__ int cell_of(float v, float inv_cs) { return (int)floorf(v * inv_cs); }

// Squared distance with the reference's float32 evaluation order and NO fused multiply-add
// (KD_TREE::calc_dist, include/ikd-Tree/ikd_Tree.cpp:1273-1277, compiled without FMA contraction; laserMapping.cpp:152-155).
__device__ __forceinline__ float dist2_ref(float qx, float qy, float qz, float px, float py, float pz) {
  float dx = __fsub_rn(qx, px), dy = __fsub_rn(qy, py), dz = __fsub_rn(qz, pz);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// The block-table probe and the cell lookup: [start, end) of cell (ix, iy, iz) in the point array (empty -> start == end); entry = the
// cell's entry index (block id * 512 + local cell; -1: the block is not in the table).
// FRESH: blocks may be CREATED beside this lookup, in the same launch (k_add_fold8<true, true>: the inserts' cells ride in the fold).  A block
// whose key is there and whose id is not yet (pad == 0; k_ins_cells' creator stores key -> id -> pad, the pad with release order) is a block
// of this very launch: it holds no point yet - empty, like a block that is not in the table.  id and pad are ONE aligned 8-byte word: a copy
// of the entry that shows pad = 1 shows the id that was stored before it, however old the copy of the key beside it is.
template <bool FRESH = false>
__device__ __forceinline__ uint2 cell_range(const GridView& g, int ix, int iy, int iz, long long& entry) {
  const int bb = kCellBias >> kCoarseShift;
  const int bx = (ix >> kCoarseShift) + bb, by = (iy >> kCoarseShift) + bb, bz = (iz >> kCoarseShift) + bb;
  const unsigned long long bk = pack_block(bx, by, bz);
  unsigned int sl = hash_block(bx, by, bz) & g.block_mask;
  while (true) {
    BlockEntry e = g.blocks[sl];
    if (e.key == bk) {
      if (FRESH && e.pad == 0u) { entry = -1; return make_uint2(0u, 0u); }
      entry = (long long)e.id * kBlockCells + local_cell(ix, iy, iz);
      return g.cells[(size_t)entry];
    }
    if (e.key == kEmptyKey) { entry = -1; return make_uint2(0u, 0u); }
    sl = (sl + 1) & g.block_mask;
  }
}
template <bool FRESH = false>
__device__ __forceinline__ uint2 cell_range(const GridView& g, int ix, int iy, int iz) {  // (for a caller that has no use for the entry index)
  long long entry;
  return cell_range<FRESH>(g, ix, iy, iz, entry);
}

// where cell entry `e` (block id * 512 + local cell) sits in the dense window that WinKeep keeps current
__device__ __forceinline__ long long win_index_of_entry(const WinKeep& w, unsigned int e) {  // -1: outside the window
  const int bb = kCellBias >> kCoarseShift;
  unsigned int kx, ky, kz;
  unpack_block(w.key_of_id[e >> 9], kx, ky, kz);
  const int bx = (int)kx - bb, by = (int)ky - bb, bz = (int)kz - bb;
  const unsigned int l = e & 511u;
  const unsigned int ux = (unsigned)(bx * 8 + (int)(l & 7u) - w.x0), uy = (unsigned)(by * 8 + (int)((l >> 3) & 7u) - w.y0), uz = (unsigned)(bz * 8 + (int)(l >> 6) - w.z0);
  if (ux < (unsigned)w.nx && uy < (unsigned)w.ny && uz < (unsigned)w.nz) return ((long long)uz * w.ny + uy) * w.nx + ux;
  return -1;
}

}  // namespace lii
