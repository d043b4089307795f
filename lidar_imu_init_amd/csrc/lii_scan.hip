// Scan pre-processing of libliinit_hip for gfx950: de-skew (IMU back-propagation / constant-velocity model) and the voxel-grid
// down-sampling, i.e. everything between the arrival of a scan and its registration.  Reference code replaced:
//   k_time_extent / k_undistort_imu / _cv ... src/IMU_Processing.hpp:390-414 and :246-266
//   k_voxel_* / k_vhash_*                    pcl::VoxelGrid::filter call site src/laserMapping.cpp:917-919 (hashed filter; the
//                                            sample-sort form lives in lii_vsort.hip)
#include <hip/hip_runtime.h>
#include <string.h>
#include <cstring>
#include <math.h>
#include <stdint.h>

#include "lii_device.h"
#include "lii_imu_dev.h"
#include "lii_launch.h"

namespace lii {

// Measurement builds (-DLII_FRONT_TRACE, tools/ab_build.sh): where the time of a de-skew and of an emit workgroup goes - 100 MHz stamps
// taken by thread 0 of every scan workgroup behind the phases named below, kept in LDS and added up at the workgroup's end as
// "ticks since the workgroup's first stamp", read back by lii_destroy.  A stamp marked W first waits for the wavefront's outstanding
// loads and atomics (vmcnt(0)): it says when the data was there, and it serialises what the product build may overlap - the table
// prices the chain of thread 0's wavefront, not the launch.
//   [0] de-skew workgroups; [1 + k]: 0 start (gated form: the record's tag seen), 1 point loaded W, 2 pose times / record in LDS,
//       3 head found, 4 point de-skewed, 5 bounding-box row written, 6 CAS returned W, 7 end; [9] the gated form's wait for the tag
//   [16] emit workgroups; [17 + k]: 0 start, 1 point and slot number back W, 2 slot line back W, 3 box folded, 4 count published,
//        6 lower counts collected, 7 end W (centroid stored)
#ifdef LII_FRONT_TRACE
__device__ unsigned long long g_front_trace[32];
__device__ __forceinline__ long long* ft_lds() {
  __shared__ long long s_ft[8];
  return s_ft;
}
#define LII_FT(k) do { if (threadIdx.x == 0) ft_lds()[k] = wall_clock64(); } while (0)
#define LII_FT_W(k) do { if (threadIdx.x == 0) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); ft_lds()[k] = wall_clock64(); } } while (0)
// (thread 0 alone: a stamp the workgroup did not take repeats the one before it)
__device__ __forceinline__ void ft_flush(int base) {
  if (threadIdx.x != 0) return;
  const long long* s = ft_lds();
  atomicAdd(&g_front_trace[base], 1ull);
  long long last = s[0];
  for (int k = 1; k < 8; k++) {
    if (s[k] != 0) last = s[k];
    atomicAdd(&g_front_trace[base + 1 + k], (unsigned long long)(last - s[0]));
  }
}
__device__ __forceinline__ void ft_begin() {
  if (threadIdx.x != 0) return;
  for (int k = 1; k < 8; k++) ft_lds()[k] = 0;
  ft_lds()[0] = wall_clock64();
}
#define LII_FT_BEGIN() ft_begin()
#define LII_FT_END(base) ft_flush(base)
void front_trace_read(unsigned long long out[32]) { (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_front_trace), sizeof(unsigned long long) * 32); }
#else
#define LII_FT(k)
#define LII_FT_W(k)
#define LII_FT_BEGIN()
#define LII_FT_END(base)
#endif

// ------------------------------------------------------------------------------------------------
// undistortion
// extent[0] = (ord(t_min) << 32) | index of the first point with that time ; extent[1] = ord(t_max)
// grid-stride over a small grid, wave shuffle + LDS reduction, ONE pair of atomics per block
// copy_to != nullptr: the scan is adopted from a caller-owned device buffer on the way (lii_scan_set_device) - one pass
// and one launch instead of a copy followed by the reduction.
__global__ __launch_bounds__(256) void k_time_extent(const float4* __restrict__ pts, int n, unsigned long long* __restrict__ extent,
                                                     unsigned long long* __restrict__ extent_next, float4* __restrict__ copy_to,
                                                     const uint4* __restrict__ ctrl_src, uint4* __restrict__ ctrl_dst, int ctrl_vec) {
  __shared__ unsigned long long smn[4], smx[4];
  // first kernel of a scan: one extra workgroup pulls the update's control block + IMU pose table out of the caller-side
  // pinned buffer (ctrl_vec 16-byte words over PCIe, ~3 us beside the others' work instead of an H2D copy submission of
  // ~10 us before the launch)
  const int n_scan_blocks = gridDim.x - (ctrl_vec > 0 ? 1 : 0);
  if ((int)blockIdx.x == n_scan_blocks) {
    for (int i0 = threadIdx.x; i0 < ctrl_vec; i0 += 256 * 4) {  // four PCIe reads in flight per lane
      uint4 v[4];
#pragma unroll
      for (int u = 0; u < 4; u++) v[u] = i0 + 256 * u < ctrl_vec ? ctrl_src[i0 + 256 * u] : make_uint4(0, 0, 0, 0);
#pragma unroll
      for (int u = 0; u < 4; u++)
        if (i0 + 256 * u < ctrl_vec) ctrl_dst[i0 + 256 * u] = v[u];
    }
    return;
  }
  // the accumulators ping-pong between two buffers: this launch re-arms the one the NEXT scan will reduce into (nobody reads
  // it any more: its consumers belonged to the previous scan), which saves a separate initialisation launch per scan
  if (blockIdx.x == 0 && threadIdx.x == 0) { extent_next[0] = ~0ull; extent_next[1] = 0ull; }
  unsigned long long mn = ~0ull, mx = 0;
  // (two points per lane and trip, both loads in flight together: the launch is sized for two points per lane)
  const int stride = n_scan_blocks * blockDim.x;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += 2 * stride) {
    const int i1 = i + stride;
    const float4 p0 = pts[i];
    const float4 p1 = pts[i1 < n ? i1 : i];
    if (copy_to) {
      copy_to[i] = p0;
      if (i1 < n) copy_to[i1] = p1;
    }
    const unsigned int o0 = f2ord(p0.w), o1 = f2ord(p1.w);
    const unsigned long long a0 = ((unsigned long long)o0 << 32) | (unsigned)i;
    const unsigned long long a1 = i1 < n ? (((unsigned long long)o1 << 32) | (unsigned)i1) : ~0ull;
    mn = a0 < mn ? a0 : mn;
    mn = a1 < mn ? a1 : mn;
    mx = (unsigned long long)o0 > mx ? (unsigned long long)o0 : mx;
    mx = (i1 < n && (unsigned long long)o1 > mx) ? (unsigned long long)o1 : mx;
  }
  for (int off = 32; off > 0; off >>= 1) {
    unsigned long long a = __shfl_xor(mn, off), b = __shfl_xor(mx, off);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  if ((threadIdx.x & 63) == 0) { smn[threadIdx.x >> 6] = mn; smx[threadIdx.x >> 6] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; w++) { mn = smn[w] < mn ? smn[w] : mn; mx = smx[w] > mx ? smx[w] : mx; }
    atomicMin(&extent[0], mn);
    atomicMax(&extent[1], mx);
  }
}
// ------------------------------------------------------------------------------------------------
// the time sort of a scan (lii_scan_job::scan_sorted == 2, lii_scan_sort; src/IMU_Processing.hpp:209, :287): key launch ->
// sort_pairs_u32 (lii_sort.hip; an LSD radix sort is stable and the value is the input index: equal keys keep their input order)
// -> gather launch.
// key[i] = the order-preserving image of t, idx[i] = i.  The reference compares floats: -0.0f == +0.0f, so the two must not be
// told apart by the key (f2ord alone would put -0.0 first) - the KEY is canonicalised, the point travels as it is.
__global__ __launch_bounds__(256) void k_sort_keys(const float4* __restrict__ pts, int n, unsigned int* __restrict__ key, unsigned int* __restrict__ idx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned int u = __float_as_uint(pts[i].w);
  if ((u << 1) == 0u) u = 0u;  // (-0.0 -> +0.0)
  key[i] = f2ord(__uint_as_float(u));
  idx[i] = (unsigned int)i;
}
// dst[i] = src[idx[i]], all four floats as they are.  Never in place: dst is another buffer than src.
// INT: the scan carries intensities (lii_scan_intensity_*): they move by the same idx, inten_dst another buffer than inten_src.
template <bool INT>
__global__ __launch_bounds__(256) void k_sort_gather(const float4* __restrict__ src, const unsigned int* __restrict__ idx, int n, float4* __restrict__ dst,
                                                     const float* __restrict__ inten_src, float* __restrict__ inten_dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned int j = idx[i];
  if (j < (unsigned int)n) {  // (idx is a permutation of 0 .. n - 1: the sort only moves what k_sort_keys wrote)
    dst[i] = src[j];
    if (INT) inten_dst[i] = inten_src[j];
  }
}
// (f2ord, ord2f and exp_so3 - Exp(ang_vel, dt), include/so3_math.h:37-59 - live in lii_device.h: lii_imu.hip shares them)
struct UndistArg {
  double endR[9], endp[3], RLI[9], TLI[3];
};

// One back-propagation step of point p with pose-table head `h` (src/IMU_Processing.hpp:398-411)
__device__ __forceinline__ void backprop_once(const double* __restrict__ head /*22 doubles*/, double t, const UndistArg& u,
                                              double p[3]) {
  double dt = t - head[0];
  const double* acc = head + 1;
  const double* gyr = head + 4;
  const double* vel = head + 7;
  const double* pos = head + 10;
  const double* rot = head + 13;
  double E[9], Ri[9];
  exp_so3(gyr, dt, E);
  mat3_mul(rot, E, Ri);
  double Pi[3];
#pragma unroll
  for (int a = 0; a < 3; a++) Pi[a] = pos[a] + vel[a] * dt + 0.5 * acc[a] * dt * dt;
  double q[3], w[3], e[3], o[3];
  mat3_vec(u.RLI, p, q);
#pragma unroll
  for (int a = 0; a < 3; a++) q[a] += u.TLI[a];
  mat3_vec(Ri, q, w);
#pragma unroll
  for (int a = 0; a < 3; a++) w[a] = w[a] + Pi[a] - u.endp[a];
  mat3t_vec(u.endR, w, e);
#pragma unroll
  for (int a = 0; a < 3; a++) e[a] -= u.TLI[a];
  mat3t_vec(u.RLI, e, o);
  p[0] = o[0]; p[1] = o[1]; p[2] = o[2];
}

// Minimum / maximum over the wavefront on DPP row operations (lii_fit.hip: wave_min_f32 - ~60 cycles where six rounds of __shfl_xor,
// LDS permutes, take ~700): lane 63 ends up with the result, the other lanes with partial ones.  Every lane of the wavefront must be
// active.  min and max of unsigned integers: exact in any order.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned int bbox_dpp(unsigned int v) {
  return (unsigned int)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, ROW_MASK, 0xF, false);
}
__device__ __forceinline__ unsigned int wave_min_to_lane63(unsigned int x) {
  x = min(x, bbox_dpp<0xB1, 0xF>(x));    // quad_perm [1, 0, 3, 2]
  x = min(x, bbox_dpp<0x4E, 0xF>(x));    // quad_perm [2, 3, 0, 1]
  x = min(x, bbox_dpp<0x141, 0xF>(x));   // row_half_mirror
  x = min(x, bbox_dpp<0x140, 0xF>(x));   // row_mirror: every lane of a row of 16 holds the row's minimum
  x = min(x, bbox_dpp<0x142, 0xA>(x));   // row_bcast15 into rows 1 and 3
  x = min(x, bbox_dpp<0x143, 0xC>(x));   // row_bcast31 into rows 2 and 3
  return x;
}
__device__ __forceinline__ unsigned int wave_max_to_lane63(unsigned int x) {
  x = max(x, bbox_dpp<0xB1, 0xF>(x));
  x = max(x, bbox_dpp<0x4E, 0xF>(x));
  x = max(x, bbox_dpp<0x141, 0xF>(x));
  x = max(x, bbox_dpp<0x140, 0xF>(x));
  x = max(x, bbox_dpp<0x142, 0xA>(x));
  x = max(x, bbox_dpp<0x143, 0xC>(x));
  return x;
}
// Bounding box of the points a 256-lane workgroup holds (non-finite points excluded; order-preserving uints): DPP reduction per
// wavefront + LDS; afterwards lanes 0..2 hold the min / max of axis threadIdx.x in lo[0] / hi[0].  Every lane must call it.
__device__ __forceinline__ void block_bbox_reduce(unsigned int (&lo)[3], unsigned int (&hi)[3]) {
  __shared__ unsigned int s_lo[4][3], s_hi[4][3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    lo[a] = wave_min_to_lane63(lo[a]);
    hi[a] = wave_max_to_lane63(hi[a]);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 63) {
#pragma unroll
    for (int a = 0; a < 3; a++) { s_lo[wave][a] = lo[a]; s_hi[wave][a] = hi[a]; }
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int a = threadIdx.x;
    lo[0] = min(min(s_lo[0][a], s_lo[1][a]), min(s_lo[2][a], s_lo[3][a]));
    hi[0] = max(max(s_hi[0][a], s_hi[1][a]), max(s_hi[2][a], s_hi[3][a]));
  }
}
__device__ __forceinline__ void bbox_point(float x, float y, float z, unsigned int (&lo)[3], unsigned int (&hi)[3]) {
  if (isfinite(x) && isfinite(y) && isfinite(z)) {
    const unsigned int ox = f2ord(x), oy = f2ord(y), oz = f2ord(z);
    lo[0] = min(lo[0], ox); hi[0] = max(hi[0], ox);
    lo[1] = min(lo[1], oy); hi[1] = max(hi[1], oy);
    lo[2] = min(lo[2], oz); hi[2] = max(hi[2], oz);
  }
}
// The de-skew kernels leave the bounding box of their output behind for the voxel filter that follows (a pass of its own
// over the scan costs a launch): one row of 8 uints per workgroup (min xyz, -, max xyz, -), reduced by k_voxel_keys.
// (Folding the rows with atomics instead costs the kernel ~5 us: 400 workgroups x 6 atomics on one cache line.)
__device__ __forceinline__ void deskew_bbox(float4 q, bool in_range, unsigned int* __restrict__ rows, int row) {
  if (!rows) return;  // uniform
  unsigned int lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0, 0, 0};
  if (in_range) bbox_point(q.x, q.y, q.z, lo, hi);
  block_bbox_reduce(lo, hi);
  if (threadIdx.x < 3) {
    rows[row * 8 + threadIdx.x] = lo[0];
    rows[row * 8 + 4 + threadIdx.x] = hi[0];
  }
}
__device__ __forceinline__ void deskew_bbox(float4 q, bool in_range, unsigned int* __restrict__ rows) { deskew_bbox(q, in_range, rows, (int)blockIdx.x); }

// The table of the hashed voxel filter (its kernels further down): open addressing, ONE 64-byte line per slot - the insert's
// CAS, atomicMin, atomicAdd and member store and the emit's reads all touch that one line (round 3 kept five parallel arrays:
// five lines per voxel).
constexpr unsigned int kVhEmpty = 0xFFFFFFFFu;
constexpr int kVhMembers = 10;  // the first arrivals of a voxel (its creator included) sit in the slot itself
struct __attribute__((aligned(64))) VhSlot {
  // The first 16 bytes decide who OWNS the voxel (min(first, creator)); the emit launch reads them with one 16-byte load and the
  // owner hands the slot back with one 16-byte store, so that a lane which looks at the slot while its owner is already freeing
  // it sees either the state before or the state after - never `first` of one and `creator` of the other (round 4 kept the creator
  // in the second 16 bytes: a lane that saw the first half old and the second half freed took itself for the owner of a
  // two-point voxel without members.  Rare - the two loads of a lane are cycles apart - until four processes time-shared one device).
  unsigned long long key;  // all ones = free.  Fused form: packed absolute voxel coordinates; separate form: the PCL voxel index
  unsigned int first;      // smallest point index among the LATER arrivals of the voxel (atomicMin); kVhEmpty: none
  unsigned int creator;    // the point that created the slot (member 0); kVhEmpty in a free slot
  unsigned int count;      // later arrivals so far (atomicAdd): the voxel holds count + 1 points
  unsigned int head;       // arrivals beyond kVhMembers: a list through next[]; kVhEmpty = none
  unsigned int members[kVhMembers - 1];  // [k - 1]: the k-th later arrival
  unsigned int pad;
};
static_assert(sizeof(VhSlot) == 64, "one cache line per slot");
struct VhTable {
  VhSlot* slots;
  unsigned int mask;        // slots - 1
  unsigned int* slot_of;    // per input point: its voxel's slot (kVhEmpty: a non-finite point, dropped as PCL drops it)
  unsigned int* next;       // per input point: list link of a crowded voxel
  unsigned int* crowded;    // one word: the longest list behind a slot so far
  // A job whose ranks share the filter by VOXEL (lii_comm_set_partition(h, 2), fused form only): part_world > 1, and a voxel whose
  // key does not hash to part_rank is none of this rank's business - its points are not inserted (voxel_rank below).
  unsigned int part_world, part_rank;
  int part_bound;           // ... and the down-sampled cloud of this rank may hold this many points (the launches behind are sized for it)
  int* part_overflow;       // ... or this word (mapped host memory) is set: the update reports LII_ERR_CAPACITY
};
__device__ __forceinline__ unsigned long long vh_mix(unsigned long long hk) {
  hk ^= hk >> 33; hk *= 0xFF51AFD7ED558CCDull; hk ^= hk >> 33;
  return hk;
}
// Which rank of a voxel-partitioned job owns a voxel: the upper half of the key's hash scaled to [0, world) - the lower half picks
// the slot.  A hash, not a range of keys: whatever the scene, every rank gets 1 / world of the voxels (+- a percent), and the
// launches behind the filter take as long as their largest share.
__device__ __forceinline__ unsigned int voxel_rank(unsigned long long key, unsigned int world) {
  return (unsigned int)(((vh_mix(key) >> 32) * (unsigned long long)world) >> 32);
}
// A point joins its voxel: the slot is found - or created - by a CAS on the key.  The point that CREATES the slot (no key there
// before) becomes entry 0 of the member list with a plain store and is done: one atomic for the ~95 % of the points of a leaf
// matched to the sensor that stay alone in their voxel - the atomics of the insert, performed at the memory side, are what the
// de-skew launch waits for (100 k of them ~ 5 us).  Only a LATER arrival pays for the bookkeeping: its arrival number (atomicAdd),
// its member entry, and the smallest index among the later arrivals (atomicMin).  The voxel's owner - its first point in input
// order - is min(creator, `first`), which the emit launch evaluates when every point has arrived; it also puts the members in
// input order.  (Round 3: CAS + atomicMin per point here and a launch of its own, k_vhash_link, to collect the members.)
// In two halves, so that a caller can put work of its own between the issue of the first CAS and the use of its result (the de-skew
// kernels: the bounding-box reduction runs while the atomic travels): vh_insert_begin issues the CAS on the key's home slot,
// vh_insert_end takes its outcome and does everything else.  The atomics a point performs, and their order, are those of the one loop.
struct VhPending {
  unsigned long long key, prev;
  unsigned int slot;
  bool active;  // false: nothing was issued (a non-finite point, another rank's voxel, a lane without a point)
};
__device__ __forceinline__ VhPending vh_insert_begin(const VhTable& tb, unsigned long long key) {
  VhPending pd;
  pd.key = key;
  pd.slot = (unsigned int)vh_mix(key) & tb.mask;
  pd.prev = atomicCAS(&tb.slots[pd.slot].key, ~0ull, key);
  pd.active = true;
  return pd;
}
__device__ __forceinline__ void vh_insert_end(const VhTable& tb, const VhPending& pd, int i) {
  const unsigned long long key = pd.key;
  unsigned int slot = pd.slot;
  unsigned long long prev = pd.prev;
  bool created;
  for (;;) {  // the table has four times as many slots as there are points: a free slot always turns up
    created = prev == ~0ull;
    if (created || prev == key) break;
    slot = (slot + 1u) & tb.mask;
    prev = atomicCAS(&tb.slots[slot].key, ~0ull, key);
  }
  VhSlot* s = tb.slots + slot;
  if (created) {
    s->creator = (unsigned)i;
  } else {
    atomicMin(&s->first, (unsigned)i);
    const unsigned int k = atomicAdd(&s->count, 1u) + 1u;
    if (k < (unsigned)kVhMembers) s->members[k - 1u] = (unsigned)i;
    else {
      tb.next[i] = atomicExch(&s->head, (unsigned)i);
      // (the watch that changes the handle over to the sort must see the same number on every rank: a rank that holds a share of
      // the voxels does not feed it)
      if (tb.part_world <= 1u) atomicMax(tb.crowded, k + 1u - (unsigned)kVhMembers);
    }
  }
  tb.slot_of[i] = slot;
}
__device__ __forceinline__ void vh_insert(const VhTable& tb, unsigned long long key, int i) { vh_insert_end(tb, vh_insert_begin(tb, key), i); }
// The insert of the fused form.  The grid PCL lays over the cloud starts at the cloud's bounding box, which is only known when
// every point has been de-skewed - but which points share a voxel is not: floor(x / leaf) decides it (PCL's index is
// floor(x * inv_leaf) - min_b, the same classes).  So the table is keyed by the absolute voxel coordinates (three 21-bit fields
// around a bias of 2^20: +- 52 km at a 5 cm leaf), and the PCL index of a voxel - the key the output is ordered by on the host -
// is computed by k_vhash_emit<true>, which knows the box.  A point outside the 21-bit range is a voxel of its own.
// Two halves like vh_insert: _begin issues the point's first CAS (`has_point` false: a lane beyond the scan, nothing happens), _end
// settles it.  Every lane of the workgroup may call both.
__device__ __forceinline__ VhPending vhash_insert_abs_begin(const float4 P, int i, bool has_point, float leaf, const VhTable& tb) {
  VhPending pd;
  pd.key = 0ull; pd.prev = 0ull; pd.slot = 0u; pd.active = false;
  if (!has_point) return pd;
  if (isfinite(P.x) && isfinite(P.y) && isfinite(P.z)) {  // (non-finite points are dropped, as PCL drops them)
    const float inv_leaf = 1.0f / leaf;
    const float fx = floorf(P.x * inv_leaf), fy = floorf(P.y * inv_leaf), fz = floorf(P.z * inv_leaf);
    unsigned long long key;
    if (fabsf(fx) < 1048000.f && fabsf(fy) < 1048000.f && fabsf(fz) < 1048000.f) {
      key = ((unsigned long long)(unsigned)((int)fz + (1 << 20)) << 42) | ((unsigned long long)(unsigned)((int)fy + (1 << 20)) << 21) |
            (unsigned long long)(unsigned)((int)fx + (1 << 20));
    } else {
      key = (1ull << 63) | (unsigned long long)(unsigned)i;
    }
    if (!(tb.part_world > 1u && voxel_rank(key, tb.part_world) != tb.part_rank)) return vh_insert_begin(tb, key);  // (else: another rank's voxel)
  }
  tb.slot_of[i] = kVhEmpty;
  return pd;
}
__device__ __forceinline__ void vhash_insert_abs_end(const VhPending& pd, int i, const VhTable& tb) {
  if (pd.active) vh_insert_end(tb, pd, i);
}

// What the two de-skew kernels share.  `in` is the scan as it arrived - the caller's device buffer (lii_scan_job::scan_dev:
// the de-skew reads it in place, round 3 copied it first) or the library's own (`out`).  sorted != 0: the points come in ascending
// time order (lii_scan_job::scan_sorted - the order the reference's preprocess hands every scan over in): the time-earliest point
// is the first, the sweep ends with the last, and the reduction that used to find them (k_time_extent, a launch of its own)
// is not needed; otherwise `extent` holds its result.  One EXTRA workgroup (ctrl_vec > 0) pulls the update's control block out
// of the caller-side pinned buffer over PCIe beside the others' work - nothing in this launch waits for it.
struct DeskewIo {
  const float4* in;
  float4* out;
  int n;
  int sorted;
  const unsigned long long* extent;
  unsigned int* bbox_rows;
  float leaf;       // FUSE: the voxel filter that follows
  VhTable tb;
  const uint4* ctrl_src;
  uint4* ctrl_dst;
  int ctrl_vec;
#ifdef LII_GAP_TRACE
  unsigned long long* gap;
#endif
};
// Measurement builds (-DLII_GAP_TRACE): how long the device sat idle between the end of the pass that stopped the previous scan's
// loop (k_reduce_solve leaves a wall_clock64 stamp, 100 MHz) and the first instruction of this scan's first kernel - the host's
// share of the scan period, measured where it is paid.  Sum and count are read back by lii_destroy.
__device__ __forceinline__ void gap_trace(const DeskewIo& io) {
#ifdef LII_GAP_TRACE
  if (blockIdx.x == 0 && threadIdx.x == 0 && io.gap) {
    const unsigned long long now = wall_clock64(), prev = io.gap[200];
    // (gaps of 50 us and more - the host did something else between two scans: the bench's bookkeeping between its regions, a
    // first-time allocation - are counted apart: the mean is over the back-to-back scans)
    if (prev != 0ull && now > prev) {
      if (now - prev < 5000ull) { io.gap[201] += now - prev; io.gap[202] += 1ull; }
      else io.gap[203] += 1ull;
    }
    io.gap[200] = 0ull;
  }
#endif
}
__device__ __forceinline__ void pull_ctrl(const DeskewIo& io) {
  for (int i0 = threadIdx.x; i0 < io.ctrl_vec; i0 += 256 * 4) {  // four PCIe reads in flight per lane
    uint4 v[4];
#pragma unroll
    for (int u = 0; u < 4; u++) v[u] = i0 + 256 * u < io.ctrl_vec ? io.ctrl_src[i0 + 256 * u] : make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int u = 0; u < 4; u++)
      if (i0 + 256 * u < io.ctrl_vec) io.ctrl_dst[i0 + 256 * u] = v[u];
  }
}
// The IMU pose table of a scan (K x 22 doubles) BY VALUE in the kernel arguments: the host writes the argument block straight
// into device memory when it enqueues the launch, so the table is there when the first wavefront starts - round 3 staged it in
// pinned memory and had the scan's first kernel pull it over PCIe, which made that kernel a launch the de-skew had to wait for.
// KP = 0: the table is in device memory (poses_g; tables beyond the largest argument block, stand-alone lii_undistort_imu).
template <int KP>
struct PoseTab { double v[KP > 0 ? KP * 22 : 1]; };

// IMU-mode de-skew.  The reference walks the time-sorted cloud backwards over the pose table; per point this
// is: head = the LAST pose index h <= K-2 with offset_time[h] < t (strict) — points with no such head stay
// untouched.  Quirk A3: the time-earliest point (first of the sorted cloud) is re-tested against every earlier
// head after being compensated, so it is compensated once per qualifying head, in descending order.
// FUSE: the de-skewed point goes straight into the table of the hashed voxel filter (vhash_insert_abs) - the filter's own
// insert launch is saved (lii_scan_register, hashed filter).
template <bool FUSE>
__device__ __forceinline__ void deskew_imu_point(const DeskewIo& io, const UndistArg& u, int K, const double* __restrict__ poses, int row, int i, bool in_range,
                                                 float4 P);
template <bool FUSE, int KP>
__global__ __launch_bounds__(256) void k_deskew_imu(DeskewIo io, UndistArg u, int K, const double* __restrict__ poses_g, PoseTab<KP> tab) {
  const int n_scan_blocks = gridDim.x - (io.ctrl_vec > 0 ? 1 : 0);
  gap_trace(io);
  if ((int)blockIdx.x == n_scan_blocks) { pull_ctrl(io); return; }
  const double* __restrict__ poses = KP > 0 ? tab.v : poses_g;
  LII_FT_BEGIN();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in_range = i < io.n;
  float4 P = in_range ? io.in[i] : make_float4(0, 0, 0, 0);
  LII_FT_W(1);
  deskew_imu_point<FUSE>(io, u, K, poses, (int)blockIdx.x, i, in_range, P);
}
// The form behind k_imu_propagate (lii_imu.hip; lii_scan_register_imu): end pose, extrinsic, number of poses and the table come from
// device memory, where that launch left them (u_g: the first 24 doubles of the propagated state).
template <bool FUSE>
__global__ __launch_bounds__(256) void k_deskew_imu_dev(DeskewIo io, const UndistArg* __restrict__ u_g, const int* __restrict__ k_g, const double* __restrict__ poses_g) {
  gap_trace(io);
  LII_FT_BEGIN();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in_range = i < io.n;
  float4 P = in_range ? io.in[i] : make_float4(0, 0, 0, 0);
  const UndistArg u = *u_g;
  const int K = *k_g;
  LII_FT_W(1);
  deskew_imu_point<FUSE>(io, u, K, poses_g, (int)blockIdx.x, i, in_range, P);
}
__device__ __forceinline__ double readlane_f64(double v, int lane /* uniform */) {
  const long long b = __double_as_longlong(v);
  const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)b, lane), hi = (unsigned int)__builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
template <bool FUSE>
__device__ __forceinline__ void deskew_imu_point(const DeskewIo& io, const UndistArg& u, int K, const double* __restrict__ poses, int row, int i, bool in_range,
                                                 float4 P) {
  // the head search walks the table's time column backwards: staged in LDS once per workgroup (tables of up to 256 poses;
  // longer ones are walked in global memory), a walk of up to K dependent global loads per point otherwise
  __shared__ double s_time[256];
  const bool staged = K <= 256;
  if (staged) {
    if ((int)threadIdx.x < K) s_time[threadIdx.x] = poses[22 * threadIdx.x];
    __syncthreads();
  }
  LII_FT(2);
  bool moved = false;
  const double t = P.w / double(1000);
  // The head of a WAVEFRONT.  The head of a time is the last k <= K - 2 with time > s_time[k]: the highest bit of a ballot in which lane k
  // holds pose k's time (tables of up to 65 poses).  It does not decrease as the time grows, so where the wavefront's first and last
  // point have the same head and every point's time lies between theirs - the scans arrive time-sorted: all but the few wavefronts
  // that straddle a pose time - that head is every point's, found with one LDS read instead of a walk of up to K - 1 dependent ones.
  // Any other wavefront (a pose time inside it, points out of order, a time that is not a number) walks as before.
  int h = -1;
  bool wave_head = false;
  if (staged && K >= 2 && K <= 65) {  // (uniform)
    const int lane = threadIdx.x & 63;
    const unsigned long long have = __ballot(in_range);
    if (have != 0ull) {
      const int l_first = __ffsll((long long)have) - 1, l_last = 63 - __clzll((long long)have);
      const double t_first = readlane_f64(t, l_first), t_last = readlane_f64(t, l_last);
      const bool pose_lane = lane <= K - 2;
      const double tk = s_time[pose_lane ? lane : 0];
      const unsigned long long b_first = __ballot(pose_lane && t_first > tk), b_last = __ballot(pose_lane && t_last > tk);
      const bool between = !in_range || (t >= t_first && t <= t_last);
      if (b_first == b_last && __all(between)) {
        wave_head = true;
        h = b_last != 0ull ? 63 - __clzll((long long)b_last) : -1;
      }
    }
  }
  if (in_range) {
    if (wave_head) {
      // (taken)
    } else if (staged) {
      for (int k = K - 2; k >= 0; k--)
        if (t > s_time[k]) { h = k; break; }
    } else {
      for (int k = K - 2; k >= 0; k--)
        if (t > poses[22 * k]) { h = k; break; }
    }
    LII_FT(3);
    if (h >= 0) {
      double p[3] = {P.x, P.y, P.z};
      backprop_once(poses + 22 * h, t, u, p);
      const bool is_begin = io.sorted ? i == 0 : ((unsigned)(io.extent[0] & 0xFFFFFFFFull) == (unsigned)i);
      if (is_begin) {
        for (int k = h - 1; k >= 0; k--) {
          if (t > poses[22 * k]) {
            // the reference reads the already-overwritten float coordinates back
            p[0] = (double)(float)p[0]; p[1] = (double)(float)p[1]; p[2] = (double)(float)p[2];
            backprop_once(poses + 22 * k, t, u, p);
          }
        }
      }
      P = make_float4((float)p[0], (float)p[1], (float)p[2], P.w);
      moved = true;
    }
    LII_FT(4);
    if (moved || io.in != io.out) io.out[i] = P;
  }
  // the point's CAS goes out first: the box reduction runs while the atomic travels to the memory side and back
  VhPending pd;
  if (FUSE) pd = vhash_insert_abs_begin(P, i, in_range, io.leaf, io.tb);
  deskew_bbox(P, in_range, io.bbox_rows, row);
  LII_FT(5);
  if (FUSE) vhash_insert_abs_end(pd, i, io.tb);
  LII_FT_W(6);
  LII_FT(7);
  LII_FT_END(0);
}

// The pre-armed form (lii_launch.h: DeskewGate).  Every workgroup requests its point, then one lane polls the tag of the record's first
// line past the caches (the host writes it last); the record goes to LDS - through the caches, every line checked against its tag -
// and the de-skew runs from there.  Workgroup 0 is the GATE - first in the grid, so that it runs whatever the launch's size: it
// watches the host's state word for CANCEL, bounds the wait (EXPIRED, by compare-and-swap), tells the others through dev_flag when
// the launch is to end without running, and pulls the update's control block once the record is there (what the extra workgroup
// of k_deskew_imu does).  A launch that does not run has written nothing.
__device__ __forceinline__ unsigned long long gate_load_u64(const void* p) {  // past the caches
  return __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
template <bool FUSE>
__global__ __launch_bounds__(256) void k_deskew_imu_gated(DeskewIo io, DeskewGate gate) {
  __shared__ unsigned long long s_verdict;
  __shared__ int s_bad, s_k;
  __shared__ double s_rec[7 * kGateLines];
  const unsigned long long armed = (gate.seq << 2) | kGateArmed, go = (gate.seq << 2) | kGateGo, cancel = (gate.seq << 2) | kGateCancel;
  const bool gate_wg = blockIdx.x == 0;
  const int row = (int)blockIdx.x - 1;
  const int i = row * (int)blockDim.x + threadIdx.x;
  const bool in_range = !gate_wg && i < io.n;
  // (requested before the wait where the scan has been in device memory all along; a scan announced while its transfer was under way -
  // late_load - is read behind the wait: the host only writes the record once the transfer is complete)
  float4 P = (in_range && !gate.late_load) ? io.in[i] : make_float4(0, 0, 0, 0);
  if (threadIdx.x == 0) {
    const long long t0 = wall_clock64();
    unsigned long long verdict = go;
    unsigned int spins = 0;
    for (;;) {
      // line 0's tag: the record is complete.  (That one tag also carries K in its top byte - the host writes it last, so the workgroup
      // knows how many lines to fetch without another load past the caches.)
      const unsigned long long t0w = gate_load_u64(gate.rec + 7);
      if ((t0w & 0x00FFFFFFFFFFFFFFull) == go) { s_k = (int)(t0w >> 56); break; }
      ++spins;
      if (gate_wg) {
        const unsigned long long w = gate_load_u64(&gate.host->word);
        if (w == cancel) { verdict = cancel; break; }
        if ((spins & 31u) == 0u) {
          // The wait is bounded WHATEVER the word holds.  A word of another sequence number is neither `cancel` nor `armed`: the host has
          // moved on to a later launch and will never write this one's record - and a word of this launch that is not `armed` any more
          // (the host's GO: it can only come while the word is armed, so before the bound) gets the bound once more for its record, which
          // the host writes right behind the GO.  Either way: one more look at the record's tag (a record that arrived in this very
          // moment stands), then the launch ends as a cancelled one.
          const long long waited = wall_clock64() - t0;
          const bool foreign = (w >> 2) != gate.seq, overdue = waited > gate.timeout_ticks;
          if (foreign || (w != armed && waited > 2 * gate.timeout_ticks)) {
            const unsigned long long t1w = gate_load_u64(gate.rec + 7);
            if ((t1w & 0x00FFFFFFFFFFFFFFull) == go) { s_k = (int)(t1w >> 56); break; }
            verdict = cancel;
            break;
          }
          if (overdue && w == armed) {
            // nobody came: EXPIRED - unless the host moves the word in this very moment, then its verdict stands (GO: the record follows)
            unsigned long long expect = armed;
            if (__hip_atomic_compare_exchange_strong(&gate.host->word, &expect, (gate.seq << 2) | kGateExpired, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE,
                                                     __HIP_MEMORY_SCOPE_SYSTEM) || expect == cancel) { verdict = cancel; break; }
          }
        }
      } else if ((spins & 3u) == 0u) {
        if (gate_load_u64(gate.dev_flag) == cancel) { verdict = cancel; break; }
        // (the gate workgroup bounds the wait; this bound - four times as long - only ends a launch whose gate never ran)
        if ((spins & 255u) == 0u && wall_clock64() - t0 > 4 * gate.timeout_ticks) { verdict = cancel; break; }
      }
      __builtin_amdgcn_s_sleep(1);
    }
    if (gate_wg && verdict == cancel) __hip_atomic_store(gate.dev_flag, cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#ifdef LII_FRONT_TRACE
    if (!gate_wg && verdict == go) atomicAdd(&g_front_trace[9], (unsigned long long)(wall_clock64() - t0));
#endif
    s_verdict = verdict;
    s_bad = 0;
  }
  __syncthreads();
  if (s_verdict != go) return;
  if (gate_wg) {
#ifdef LII_GAP_TRACE
    gap_trace(io);
#endif
    if (io.ctrl_vec > 0) pull_ctrl(io);
    return;
  }
  LII_FT_BEGIN();
  if (in_range && gate.late_load) P = io.in[i];
  LII_FT_W(1);
  // the record -> LDS
  const int K = s_k;
  const int n_lines = (25 + 22 * (K < 2 ? 2 : (K > kGateMaxPoses ? kGateMaxPoses : K)) + 6) / 7;
  for (int e = threadIdx.x; e < 8 * n_lines; e += 256) {
    const double v = gate.rec[e];
    if ((e & 7) == 7) { if (((unsigned long long)__double_as_longlong(v) & 0x00FFFFFFFFFFFFFFull) != go) s_bad = 1; }
    else s_rec[(e >> 3) * 7 + (e & 7)] = v;
  }
  __syncthreads();
  if (s_bad) {  // (uniform; rare) a line came out of a cache as an older record left it: everything again, past the caches
    for (int e = threadIdx.x; e < 8 * n_lines; e += 256)
      if ((e & 7) != 7) s_rec[(e >> 3) * 7 + (e & 7)] = __longlong_as_double((long long)gate_load_u64(gate.rec + e));
    __syncthreads();
  }
  UndistArg u;
#pragma unroll
  for (int e = 0; e < 9; e++) { u.endR[e] = s_rec[1 + e]; u.RLI[e] = s_rec[13 + e]; }
#pragma unroll
  for (int e = 0; e < 3; e++) { u.endp[e] = s_rec[10 + e]; u.TLI[e] = s_rec[22 + e]; }
  deskew_imu_point<FUSE>(io, u, K, s_rec + 25, row, i, i < io.n, P);
}

struct CvArg {
  double omega[3], vel[3], endR[9];
};
// CV-mode de-skew (src/IMU_Processing.hpp:246-266).  The time-earliest point is skipped (quirk A3).  What a scan workgroup does,
// shared by the two kernels below.
template <bool FUSE>
__device__ __forceinline__ void deskew_cv_point(const DeskewIo& io, const double (&omega)[3], const double (&rv)[3] /* endR^T vel */) {
  LII_FT_BEGIN();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in_range = i < io.n;
  float4 P = in_range ? io.in[i] : make_float4(0, 0, 0, 0);
  LII_FT_W(1);
  if (in_range) {
    const bool is_begin = io.sorted ? i == 0 : ((unsigned)(io.extent[0] & 0xFFFFFFFFull) == (unsigned)i);
    if (!is_begin) {
      // the sweep's end: the largest time stamp (sorted: the last point's)
      const float t_end = io.sorted ? io.in[io.n - 1].w : ord2f((unsigned)io.extent[1]);
      double end_off = t_end / double(1000);
      double dt_j = end_off - P.w / double(1000);
      double R[9];
      exp_so3(omega, -dt_j, R);
      double p[3] = {P.x, P.y, P.z}, o[3];
      mat3_vec(R, p, o);
#pragma unroll
      for (int c = 0; c < 3; c++) o[c] = o[c] + (-rv[c]) * dt_j;
      P = make_float4((float)o[0], (float)o[1], (float)o[2], P.w);
      io.out[i] = P;
    } else if (io.in != io.out) {
      io.out[i] = P;
    }
  }
  LII_FT(4);
  VhPending pd;  // (the CAS first, the box reduction in its shadow: deskew_imu_point)
  if (FUSE) pd = vhash_insert_abs_begin(P, i, in_range, io.leaf, io.tb);
  deskew_bbox(P, in_range, io.bbox_rows);
  LII_FT(5);
  if (FUSE) vhash_insert_abs_end(pd, i, io.tb);
  LII_FT_W(6);
  LII_FT(7);
  LII_FT_END(0);
}
template <bool FUSE>
__global__ __launch_bounds__(256) void k_deskew_cv(DeskewIo io, CvArg a) {
  const int n_scan_blocks = gridDim.x - (io.ctrl_vec > 0 ? 1 : 0);
  if ((int)blockIdx.x == n_scan_blocks) { pull_ctrl(io); return; }
  double rv[3];
  mat3t_vec(a.endR, a.vel, rv);
  deskew_cv_point<FUSE>(io, a.omega, rv);
}

// The CV de-skew that carries the propagation of the LO phase (lii_scan_register_cv): Process() with imu_en == false,
// src/IMU_Processing.hpp:212-266, in ONE launch.  The arguments hold the state as the previous update left it - not propagated.
//   scan workgroups  form the propagated end rotation themselves, rot_end * Exp(bias_g, dt) (:228, :241) - everything they need
//                    arrives by value, so they wait for nothing - and go on as k_deskew_cv does;
//   extra workgroup  the whole propagation (cv_propagate_lds, the arithmetic of k_cv_propagate: the one cov_step over P in LDS, then
//                    rotation and position).  The state comes out of the control block in pinned host memory (fill_ctrl); the
//                    propagated state goes to IekfCtrl::st and ::prop on the device - and to mapped host memory if asked - and the
//                    words of the block behind the two states are pulled over beside it.
// Its st[0..8] and the scan workgroups' end rotation are the same instructions on the same numbers: the same bits.
struct CvFuseArg {
  double rot[9], bias_g[3], vel[3];  // rot_end, bias_g, vel_end of the unpropagated state
  double dt;
  double cov_gyr_scale[3], cov_acc_scale[3];
  const double* st_in;   // the whole lii_state (pinned host memory)
  double* st_out;        // IekfCtrl::st (612 doubles)
  double* prop_out;      // IekfCtrl::prop (36 doubles)
  double* host_out;      // optional, mapped host memory (612 doubles)
  int ctrl_from;         // first 16-byte word of the control block behind the two states
};
__device__ __forceinline__ void cv_extra_workgroup(const DeskewIo& io, const CvFuseArg& f) {
  __shared__ CvPropLds L;
  const int tid = threadIdx.x;
  // (both PCIe reads under way together: the state's 612 doubles and the rest of the block)
  const double x = tid < 36 ? f.st_in[tid] : 0.0;
  const double p0 = f.st_in[36 + tid], p1 = f.st_in[36 + 256 + tid], p2 = tid < 64 ? f.st_in[36 + 512 + tid] : 0.0;
  if (io.ctrl_vec > f.ctrl_from) pull_words(io.ctrl_src, io.ctrl_dst, f.ctrl_from, io.ctrl_vec, tid, 256);
  if (tid < 36) L.x[tid] = x;
  L.P[tid] = p0;
  L.P[256 + tid] = p1;
  if (tid < 64) L.P[512 + tid] = p2;
  __syncthreads();
  cv_propagate_lds(L, f.dt, f.cov_gyr_scale, f.cov_acc_scale);
  if (tid < 36) {
    f.st_out[tid] = L.x[tid];
    f.prop_out[tid] = L.x[tid];
    if (f.host_out) f.host_out[tid] = L.x[tid];
  }
  for (int e = tid; e < 576; e += 256) {
    f.st_out[36 + e] = L.P[e];
    if (f.host_out) f.host_out[36 + e] = L.P[e];
  }
}
template <bool FUSE>
__global__ __launch_bounds__(256) void k_deskew_cv_prop(DeskewIo io, CvFuseArg f) {
  if ((int)blockIdx.x == (int)gridDim.x - 1) { cv_extra_workgroup(io, f); return; }  // (always there: the grid is the scan's workgroups + 1)
  double endR[9], rv[3];
  cv_end_rotation(f.rot, f.bias_g, f.dt, endR);
  mat3t_vec(endR, f.vel, rv);  // (the nine doubles of the rotation end here: three stay live over the per-point code)
#pragma unroll
  for (int c = 0; c < 3; c++) {  // (the same in every lane: held in scalar registers, the kernel stays at k_deskew_cv's 50 VGPRs - 68 with them in vector registers)
    const long long b = __double_as_longlong(rv[c]);
    const unsigned int lo = __builtin_amdgcn_readfirstlane((unsigned int)b), hi = __builtin_amdgcn_readfirstlane((unsigned int)(b >> 32));
    rv[c] = __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
  }
  deskew_cv_point<FUSE>(io, f.bias_g, rv);
}

// ------------------------------------------------------------------------------------------------
// voxel-grid down-sampling (PCL VoxelGrid restatement)
// mm[0..2] = ord(min xyz), mm[3..5] = ord(max xyz)
__global__ __launch_bounds__(256) void k_voxel_minmax(const float4* __restrict__ pts, int n, unsigned int* __restrict__ mm,
                                                      unsigned int* __restrict__ mm_next) {
  // grid-stride over a small grid; re-arms the ping-pong partner buffer for the next scan (see k_time_extent)
  if (blockIdx.x == 0 && threadIdx.x < 6) mm_next[threadIdx.x] = threadIdx.x < 3 ? 0xFFFFFFFFu : 0u;
  unsigned int lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0, 0, 0};
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float4 p = pts[i];
    bbox_point(p.x, p.y, p.z, lo, hi);
  }
  block_bbox_reduce(lo, hi);
  if (threadIdx.x < 3) {  // ONE set of atomics per workgroup (<= 256 of them)
    atomicMin(&mm[threadIdx.x], lo[0]);
    atomicMax(&mm[3 + threadIdx.x], hi[0]);
  }
}

struct VoxelArg {
  float inv_leaf;
  int min_b[3];
  int mul[3];
  int identity;  // PCL's int32 index-overflow guard tripped: output = input
};
// Derives the voxel-grid parameters from the min/max reduction ON THE DEVICE (no host round trip), in every thread of the
// key kernel (six loads + a few flops — cheaper than a launch of its own):
// PCL VoxelGrid::applyFilter — bounding box, (dx*dy*dz) > INT32_MAX -> "Leaf size is too small" -> identity copy.
__device__ __forceinline__ VoxelArg voxel_prepare(const unsigned int* __restrict__ mm, float leaf) {
  VoxelArg v;
  v.inv_leaf = 1.0f / leaf;
  v.identity = 0;
  for (int a = 0; a < 3; a++) { v.min_b[a] = 0; v.mul[a] = 0; }
  if (mm[0] != 0xFFFFFFFFu) {  // at least one finite point
    float mn[3], mx[3];
    for (int a = 0; a < 3; a++) {
      unsigned int lo = mm[a], hi = mm[3 + a];
      unsigned int ul = (lo & 0x80000000u) ? (lo & 0x7FFFFFFFu) : ~lo, uh = (hi & 0x80000000u) ? (hi & 0x7FFFFFFFu) : ~hi;
      mn[a] = __uint_as_float(ul);
      mx[a] = __uint_as_float(uh);
    }
    long long dx = (long long)((mx[0] - mn[0]) * v.inv_leaf) + 1, dy = (long long)((mx[1] - mn[1]) * v.inv_leaf) + 1,
              dz = (long long)((mx[2] - mn[2]) * v.inv_leaf) + 1;
    if (dx * dy * dz > 2147483647LL) {
      v.identity = 1;
    } else {
      int div_b[3];
      for (int a = 0; a < 3; a++) {
        v.min_b[a] = (int)floorf(mn[a] * v.inv_leaf);
        div_b[a] = (int)floorf(mx[a] * v.inv_leaf) - v.min_b[a] + 1;
      }
      v.mul[0] = 1; v.mul[1] = div_b[0]; v.mul[2] = div_b[0] * div_b[1];
    }
  }
  return v;
}
__global__ __launch_bounds__(256) void k_voxel_keys(const float4* __restrict__ pts, int n, const unsigned int* __restrict__ mm,
                                                    const unsigned int* __restrict__ bbox_rows, int n_rows, float leaf,
                                                    unsigned long long* __restrict__ keys, unsigned int* __restrict__ pcl_keys,
                                                    int* __restrict__ filtered,
                                                    unsigned long long* __restrict__ samples, int sample_width) {
  __shared__ unsigned int s_mm[8];
  if (n_rows > 0) {  // the box arrives as one row per de-skew workgroup: every workgroup folds them for itself (a few KB from L2)
    unsigned int lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0, 0, 0};
    for (int r = threadIdx.x; r < n_rows; r += 256) {
      const uint4 a = *reinterpret_cast<const uint4*>(bbox_rows + r * 8), b = *reinterpret_cast<const uint4*>(bbox_rows + r * 8 + 4);
      lo[0] = min(lo[0], a.x); lo[1] = min(lo[1], a.y); lo[2] = min(lo[2], a.z);
      hi[0] = max(hi[0], b.x); hi[1] = max(hi[1], b.y); hi[2] = max(hi[2], b.z);
    }
    block_bbox_reduce(lo, hi);
    if (threadIdx.x < 3) { s_mm[threadIdx.x] = lo[0]; s_mm[3 + threadIdx.x] = hi[0]; }
    __syncthreads();
    mm = s_mm;
  }
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const VoxelArg v = voxel_prepare(mm, leaf);
  if (i == 0) *filtered = v.identity ? 0 : 1;
  float4 p = pts[i];
  unsigned long long key = kVoxDropKey;  // non-finite points sort last and are dropped
  unsigned int pcl = 0x7FFFFFFFu;
  if (v.identity) {
    key = pcl = (unsigned)i;  // every point is its own voxel, in input order
  } else if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
    int i0 = (int)(floorf(p.x * v.inv_leaf) - (float)v.min_b[0]);
    int i1 = (int)(floorf(p.y * v.inv_leaf) - (float)v.min_b[1]);
    int i2 = (int)(floorf(p.z * v.inv_leaf) - (float)v.min_b[2]);
    pcl = (unsigned)(i0 * v.mul[0] + i1 * v.mul[1] + i2 * v.mul[2]);
    key = pcl;
  }
  keys[i] = key;
  pcl_keys[i] = pcl;
  if (samples) {  // the sort's splitter samples (lii_vsort.hip): one jittered position per stratum of `sample_width` points
    const unsigned int j = (unsigned int)i / (unsigned int)sample_width, lo = j * (unsigned int)sample_width;
    unsigned int hsh = j * 2654435761u;
    hsh ^= hsh >> 15; hsh *= 2246822519u; hsh ^= hsh >> 13;
    const unsigned int w = min((unsigned int)sample_width, (unsigned int)n - lo);
    if (lo + hsh % w == (unsigned int)i) samples[j] = (key << kVoxIdxBits) | (unsigned long long)(unsigned int)i;
  }
}
// ------------------------------------------------------------------------------------------------
// The voxel grid without a sort (the default path; the sample sort of lii_vsort.hip stays for crowded voxels and
// LII_VOXEL_FILTER=sort).
// PCL's filter sorts the points by voxel index only to bring the points of a voxel together and to emit the voxels in index
// order; the centroids themselves depend on the ORDER OF THE POINTS INSIDE a voxel (float sums, input order), not on the
// order of the voxels.  So the points of a voxel are brought together by a hash table instead, and the voxels leave in the
// order of their first points (the PCL index of every output voxel is kept: lii_scan_download / lii_neighbors_download put
// the reference's order back on the host).  Two launches (round 3: three), the first of which rides in the de-skew launch
// inside lii_scan_register:
//   insert          vh_insert: the voxel's slot in an open-addressing table (CAS on the key); the creator of a slot is done with
//                   that, a later arrival adds its arrival number, member entry and index minimum - k_vhash_insert keyed by
//                   the PCL voxel index, or vhash_insert_abs from the de-skew kernels keyed by absolute voxel coordinates
//   k_vhash_emit    a point is the voxel's owner when it is its first point; output position = number of owners before it -
//                   the owners of a workgroup are counted, the count is published, and the counts of the workgroups below
//                   are collected INSIDE the launch, after the owner has formed its centroid (by then they have long been
//                   published: the exchange hides behind the dependent loads of the centroid; round 3 counted in a launch of
//                   its own).  The owner puts the members in input order (ascending index) by repeated selection, adds the
//                   points in that order - the float additions of PCL's centroid - writes the centroid and frees its slot.
// Deterministic: the slot a voxel lands in and the order in which members arrive vary from run to run, neither reaches the
// output.
__global__ __launch_bounds__(256) void k_vh_clear(VhSlot* slots, unsigned int n_slots) {
  const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_slots) return;
  VhSlot s;
  s.key = ~0ull; s.first = kVhEmpty; s.creator = kVhEmpty; s.count = 0u; s.head = kVhEmpty; s.pad = 0u;
#pragma unroll
  for (int k = 0; k < kVhMembers - 1; k++) s.members[k] = kVhEmpty;
  slots[i] = s;
}
// Folds the bounding-box rows the de-skew workgroups left behind (every workgroup for itself: a few KB from L2).
__device__ __forceinline__ void fold_bbox_rows(const unsigned int* __restrict__ bbox_rows, int n_rows, unsigned int* s_mm /*[8] LDS*/) {
  unsigned int lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0, 0, 0};
  for (int r = threadIdx.x; r < n_rows; r += 256) {
    const uint4 a = *reinterpret_cast<const uint4*>(bbox_rows + r * 8), b = *reinterpret_cast<const uint4*>(bbox_rows + r * 8 + 4);
    lo[0] = min(lo[0], a.x); lo[1] = min(lo[1], a.y); lo[2] = min(lo[2], a.z);
    hi[0] = max(hi[0], b.x); hi[1] = max(hi[1], b.y); hi[2] = max(hi[2], b.z);
  }
  block_bbox_reduce(lo, hi);
  if (threadIdx.x < 3) { s_mm[threadIdx.x] = lo[0]; s_mm[3 + threadIdx.x] = hi[0]; }
  __syncthreads();
}
// The same fold in two halves (k_vhash_emit): the first two rows of a lane - scans of up to 131 072 points have no more - are REQUESTED
// with the lane's other loads, and reduced when the result is needed.  min / max: the same box whatever the order.
// (The request is written as relaxed atomic loads of wavefront scope - ordinary load instructions - because the compiler sinks an
// ordinary load to its first use, behind the publication: the rows' round trip would then start where the result is needed.)
struct BoxRows { uint4 a0, b0, a1, b1; };
__device__ __forceinline__ uint4 box_row_half(const unsigned int* p /* 16-byte aligned */) {
  const unsigned long long* q = reinterpret_cast<const unsigned long long*>(p);
  const unsigned long long u = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT), w = __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
  return make_uint4((unsigned int)u, (unsigned int)(u >> 32), (unsigned int)w, (unsigned int)(w >> 32));
}
__device__ __forceinline__ BoxRows fold_bbox_rows_request(const unsigned int* __restrict__ bbox_rows, int n_rows) {
  // (n_rows >= 1.  A lane beyond the rows reads the last one again - the box does not change, and no lane waits to choose)
  BoxRows q;
  const int r0 = min((int)threadIdx.x, n_rows - 1), r1 = min((int)threadIdx.x + 256, n_rows - 1);
  q.a0 = box_row_half(bbox_rows + r0 * 8); q.b0 = box_row_half(bbox_rows + r0 * 8 + 4);
  q.a1 = box_row_half(bbox_rows + r1 * 8); q.b1 = box_row_half(bbox_rows + r1 * 8 + 4);
  return q;
}
__device__ __forceinline__ void fold_bbox_rows_finish(const BoxRows& q, const unsigned int* __restrict__ bbox_rows, int n_rows, unsigned int* s_mm /*[8] LDS*/) {
  unsigned int lo[3] = {min(q.a0.x, q.a1.x), min(q.a0.y, q.a1.y), min(q.a0.z, q.a1.z)}, hi[3] = {max(q.b0.x, q.b1.x), max(q.b0.y, q.b1.y), max(q.b0.z, q.b1.z)};
  for (int r = threadIdx.x + 512; r < n_rows; r += 256) {
    const uint4 a = *reinterpret_cast<const uint4*>(bbox_rows + r * 8), b = *reinterpret_cast<const uint4*>(bbox_rows + r * 8 + 4);
    lo[0] = min(lo[0], a.x); lo[1] = min(lo[1], a.y); lo[2] = min(lo[2], a.z);
    hi[0] = max(hi[0], b.x); hi[1] = max(hi[1], b.y); hi[2] = max(hi[2], b.z);
  }
  block_bbox_reduce(lo, hi);
  if (threadIdx.x < 3) { s_mm[threadIdx.x] = lo[0]; s_mm[3 + threadIdx.x] = hi[0]; }
  __syncthreads();
}
__global__ __launch_bounds__(256) void k_vhash_insert(const float4* __restrict__ pts, int n, const unsigned int* __restrict__ mm,
                                                      const unsigned int* __restrict__ bbox_rows, int n_rows, float leaf,
                                                      VhTable tb, int* __restrict__ filtered) {
  __shared__ unsigned int s_mm[8];
  if (n_rows > 0) {
    fold_bbox_rows(bbox_rows, n_rows, s_mm);
    mm = s_mm;
  }
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const VoxelArg v = voxel_prepare(mm, leaf);
  if (i == 0) *filtered = v.identity ? 0 : 1;
  const float4 p = pts[i];
  unsigned long long key = ~0ull;  // non-finite points are dropped
  if (v.identity) {
    key = (unsigned)i;  // every point is its own voxel
  } else if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
    const int i0 = (int)(floorf(p.x * v.inv_leaf) - (float)v.min_b[0]);
    const int i1 = (int)(floorf(p.y * v.inv_leaf) - (float)v.min_b[1]);
    const int i2 = (int)(floorf(p.z * v.inv_leaf) - (float)v.min_b[2]);
    key = (unsigned)(i0 * v.mul[0] + i1 * v.mul[1] + i2 * v.mul[2]);  // < 2^31 (the overflow guard)
  }
  if (key != ~0ull) vh_insert(tb, key, i);
  else tb.slot_of[i] = kVhEmpty;
}
// exclusive scan over the 256 lanes of a workgroup of 0 / 1 flags; *total = flags set in the workgroup
__device__ __forceinline__ unsigned int block_rank_of_flag(bool f, unsigned int* s_w /*[4] LDS*/, unsigned int* total) {
  const unsigned long long b = __ballot(f);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s_w[wave] = (unsigned)__popcll(b);
  __syncthreads();
  unsigned int before = 0;
  for (int w = 0; w < wave; w++) before += s_w[w];
  *total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
  return before + (unsigned)__popcll(b & ((1ull << lane) - 1ull));
}
// ABS: the table was filled by the fused form (absolute voxel coordinates): the box arrives here (one row per de-skew
// workgroup, folded by every workgroup for itself), the PCL index of a voxel is computed from its first point, and PCL's
// overflow guard (the grid would have more than 2^31 voxels: "leaf size too small", the cloud passes unfiltered) is applied
// here - every point then leaves as it is, in input order.
// *crowded (written by vh_insert when a point goes to a list): the host reads it behind the filter and takes the sort path from
// then on when voxels hold dozens of points (a large leaf) - the owner orders the members by repeated selection, quadratic in
// their number.
// INT: the scan carries intensities (inten[i] beside pts[i]): the owner adds its members' in the order it adds their points - from 0.f,
// __fadd_rn, divided by the count: the `intensity` field of PCL's centroid - and writes the voxel's to inten_out at the voxel's place.  It
// has to happen here: the owner frees the slot, nobody can walk the members afterwards.  INT = false is the code without the channel.
template <bool ABS, bool INT>
__global__ __launch_bounds__(256) void k_vhash_emit(const float4* __restrict__ pts, int n, VhTable tb, unsigned long long* __restrict__ counts,
                                                    unsigned int epoch, float4* __restrict__ out, int* __restrict__ n_out,
                                                    unsigned int* __restrict__ pcl_out, const unsigned int* __restrict__ bbox_rows,
                                                    int n_rows, float leaf, int* __restrict__ filtered, int test_late,
                                                    const float* __restrict__ inten, float* __restrict__ inten_out) {
  __shared__ unsigned int s_w[4], s_sum[12];
  LII_FT_BEGIN();
  const int tid = threadIdx.x, i = blockIdx.x * blockDim.x + tid;
  // everything a lane needs of its own point is requested at once: the point, its slot, and (dependent) the slot's line
  const bool in_range = i < n;
  const float4 p0 = in_range ? pts[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  const unsigned int slot = in_range ? tb.slot_of[i] : kVhEmpty;
  const float q0 = (INT && in_range) ? inten[i] : 0.f;
  // ABS: the box.  Its fold - a reduction over the workgroup, two barriers - is needed for pcl_out and the overflow guard, not for the
  // ownership, the count or its publication: the rows are requested here with the lane's other loads and folded BEHIND the
  // publication of the count, which every workgroup above this one waits for.  Two forms need
  // the box before: a job shared by voxel (ident_part enters `first`) and LII_TEST=emit_late (`hold` reads v.identity): they fold here.
  __shared__ unsigned int s_mm[8];
  const bool fold_first = ABS && (tb.part_world > 1u || test_late != 0 || n_rows < 1);  // (uniform)
  BoxRows box_rows = {};
  if (ABS && !fold_first) box_rows = fold_bbox_rows_request(bbox_rows, n_rows);
  LII_FT_W(1);
  VoxelArg v;
  v.identity = 0;
  if (fold_first) {
    fold_bbox_rows(bbox_rows, n_rows, s_mm);
    v = voxel_prepare(s_mm, leaf);
    if (i == 0) *filtered = v.identity ? 0 : 1;
    LII_FT(3);
  }
  VhSlot* const sl = tb.slots + (slot != kVhEmpty ? slot : 0u);
  uint4 hd = make_uint4(0u, 0u, kVhEmpty, 0u), m0 = make_uint4(kVhEmpty, kVhEmpty, kVhEmpty, kVhEmpty), m1 = m0;
  uint2 m2 = make_uint2(kVhEmpty, kVhEmpty);
  unsigned long long key = 0;
  if (slot != kVhEmpty) {  // the slot's line in four requests
    const uint4* line = reinterpret_cast<const uint4*>(sl);
    const uint4 a = line[0];  // key, first, creator: ONE request decides the ownership (see VhSlot)
    key = ((unsigned long long)a.y << 32) | a.x;
    hd.x = a.z;
    m0.x = a.w;
    const uint4 b = line[1];  // count, head, members 1..2
    hd.y = b.x; hd.z = b.y;
    m0.y = b.z; m0.z = b.w;
    const uint4 c = line[2], d = line[3];  // members 3..6, 7..9 (+ padding)
    m0.w = c.x; m1 = make_uint4(c.y, c.z, c.w, d.x); m2 = make_uint2(d.y, d.z);
  }
  LII_FT_W(2);
  // (a voxel-partitioned job whose cloud passes unfiltered - PCL's overflow guard - still shares it by voxel: every point of a
  // voxel of this rank leaves on its own)
  const bool ident_part = ABS && v.identity && tb.part_world > 1u;
  const bool first = slot != kVhEmpty && (ident_part || min(hd.x, m0.x) == (unsigned)i);  // the owner: the first point of the voxel in input order
  unsigned int total;
  const unsigned int rank = block_rank_of_flag(first, s_w, &total);
  // The workgroup's count goes out BEFORE it looks at anybody else's (prefix_below, lii_device.h: the exchange of the counts inside
  // the launch, placement-independent).  LII_TEST=emit_late: every seventh workgroup holds its word back until it is done, so that
  // the workgroups above it have to count its block themselves - the path a launch takes whose workgroups are not all resident.
  const bool hold = test_late != 0 && (blockIdx.x % 7u) == 3u && !(ABS && v.identity && !ident_part);
  if (tid == 0 && !hold) __hip_atomic_store(counts + blockIdx.x, ((unsigned long long)epoch << 32) | total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  LII_FT(4);
  // (The words of the workgroups below are NOT requested here: the workgroups publish within a microsecond of each other, a look this
  // early finds most words missing and pays a second round trip where `base` is needed - measured, 1.5 us per launch, profiles/front_end.md.)
  if (ABS && !fold_first) {
    fold_bbox_rows_finish(box_rows, bbox_rows, n_rows, s_mm);
    v = voxel_prepare(s_mm, leaf);
    if (i == 0) *filtered = v.identity ? 0 : 1;
    LII_FT(3);
  }
  if (ABS && v.identity && !ident_part) {  // (uniform) the cloud passes unfiltered; the voxels' owners still hand their slots back
    if (in_range) { out[i] = p0; pcl_out[i] = (unsigned)i; }
    if (INT && in_range) inten_out[i] = q0;
    if (blockIdx.x == gridDim.x - 1 && tid == 0) *n_out = n;
    if (first) {
      uint4* line = reinterpret_cast<uint4*>(sl);
      line[0] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, kVhEmpty, kVhEmpty);
      line[1] = make_uint4(0u, kVhEmpty, kVhEmpty, kVhEmpty);
    }
    return;
  }
  float4 cen = make_float4(0.f, 0.f, 0.f, 0.f);
  float cen_i = 0.f;
  if (first) {
    const unsigned int cnt = ident_part ? 1u : hd.y + 1u;  // points of the voxel, this one included
    float sx = __fadd_rn(0.f, p0.x), sy = __fadd_rn(0.f, p0.y), sz = __fadd_rn(0.f, p0.z), st = __fadd_rn(0.f, p0.w);
    float si = INT ? __fadd_rn(0.f, q0) : 0.f;
    unsigned int m[kVhMembers] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w, m2.x, m2.y};
#pragma unroll
    for (int k = 0; k < kVhMembers; k++)
      if ((unsigned)k >= cnt) m[k] = kVhEmpty;  // (entries beyond the count are stale: the slot is not wiped member by member)
    if (cnt > 512u) {
      // Safety valve for a scan on which voxels turn crowded in the middle of a run (the first scan of a leaf is probed, the
      // following ones watched: lii_downsample): ordering hundreds of members by repeated selection would take tens of
      // milliseconds.  They are added in list order - the centroid is then right to rounding, not bit for bit.
#pragma unroll
      for (int k = 0; k < kVhMembers; k++) {
        if (m[k] == (unsigned)i || m[k] == kVhEmpty) continue;
        const float4 p = pts[m[k]];
        sx = __fadd_rn(sx, p.x); sy = __fadd_rn(sy, p.y); sz = __fadd_rn(sz, p.z); st = __fadd_rn(st, p.w);
        if (INT) si = __fadd_rn(si, inten[m[k]]);
      }
      for (unsigned int j = hd.z; j != kVhEmpty; j = tb.next[j]) {
        if (j == (unsigned)i) continue;
        const float4 p = pts[j];
        sx = __fadd_rn(sx, p.x); sy = __fadd_rn(sy, p.y); sz = __fadd_rn(sz, p.z); st = __fadd_rn(st, p.w);
        if (INT) si = __fadd_rn(si, inten[j]);
      }
    } else if (cnt > 1u) {
      // the members in input order: every round takes the smallest index above the last one taken (the owner's own index is
      // the smallest of all, so it never comes up again) - from the slot's own members (registers) and, for a crowded voxel,
      // from the list behind them (walked again every round: slow and rare)
      const unsigned int head = cnt > (unsigned)kVhMembers ? hd.z : kVhEmpty;
      unsigned int last = (unsigned)i;
      for (unsigned int r = 1; r < cnt; r++) {
        unsigned int best = kVhEmpty;
#pragma unroll
        for (int k = 0; k < kVhMembers; k++) best = (m[k] > last && m[k] < best) ? m[k] : best;
        for (unsigned int j = head; j != kVhEmpty; j = tb.next[j]) best = (j > last && j < best) ? j : best;
        const float4 p = pts[best];
        sx = __fadd_rn(sx, p.x); sy = __fadd_rn(sy, p.y); sz = __fadd_rn(sz, p.z); st = __fadd_rn(st, p.w);
        if (INT) si = __fadd_rn(si, inten[best]);
        last = best;
      }
    }
    const float c = (float)cnt;
    // a single-point voxel reproduces the point exactly (x / 1.0f == x), which is also what the identity path needs
    cen = make_float4(sx / c, sy / c, sz / c, st / c);
    if (INT) cen_i = si / c;
  }
  // owners in the workgroups below this one; a block whose word is overdue is counted here: which of its points own their voxel
  // (one 16-byte request per point decides it, as above; a slot its owner - a point of another block - has freed already reads
  // empty: not this point's voxel any more, and it never was its owner)
  const unsigned int base =
      prefix_below(counts, epoch, (int)blockIdx.x, s_sum, test_late != 0, [&](int q) -> unsigned int {
    const int j = q * 256 + tid;
    bool f = false;
    if (j < n) {
      const unsigned int sq = tb.slot_of[j];
      if (sq != kVhEmpty) {
        const uint4 a = *reinterpret_cast<const uint4*>(tb.slots + sq);
        f = ident_part || min(a.z, a.w) == (unsigned)j;
      }
    }
    unsigned int tot;
    (void)block_rank_of_flag(f, s_w, &tot);
    return tot;
  }).y;
  LII_FT(6);
  if (hold) {  // (uniform; tests only) the word must be out before ANY lane of this workgroup frees a slot: a helper that recounts this
               // block from freed slots trusts its own count only while the word is missing (prefix_below)
    if (tid == 0) {
      __hip_atomic_store(counts + blockIdx.x, ((unsigned long long)epoch << 32) | total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    }
    __syncthreads();
  }
  if (blockIdx.x == gridDim.x - 1 && tid == 0) {  // size of the down-sampled cloud
    int n_down = (int)(base + total);
    if (ABS && tb.part_world > 1u && n_down > tb.part_bound) {  // this rank's share outgrew what the launches behind are sized for
      n_down = tb.part_bound;
      __hip_atomic_store(tb.part_overflow, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    *n_out = n_down;
  }
  if (first) {
    const unsigned int pos = base + rank;
    out[pos] = cen;
    if (INT) inten_out[pos] = cen_i;
    if (ident_part) {
      pcl_out[pos] = (unsigned)i;
    } else if (ABS) {
      // PCL's index of this voxel, from any of its points (the first): as k_vhash_insert computes it
      const int i0 = (int)(floorf(p0.x * v.inv_leaf) - (float)v.min_b[0]);
      const int i1 = (int)(floorf(p0.y * v.inv_leaf) - (float)v.min_b[1]);
      const int i2 = (int)(floorf(p0.z * v.inv_leaf) - (float)v.min_b[2]);
      pcl_out[pos] = (unsigned)(i0 * v.mul[0] + i1 * v.mul[1] + i2 * v.mul[2]);
    } else {
      pcl_out[pos] = (unsigned int)key;
    }
    // the slot is free again for the next scan
    uint4* line = reinterpret_cast<uint4*>(sl);
    line[0] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, kVhEmpty, kVhEmpty);
    line[1] = make_uint4(0u, kVhEmpty, kVhEmpty, kVhEmpty);
  }
  LII_FT_W(7);
  LII_FT_END(16);
}

// ------------------------------------------------------------------------------------------------
// launchers
static inline int nblk(int n, int b) { return (n + b - 1) / b; }
void launch_time_extent(const float4* pts, int n, unsigned long long* extent, unsigned long long* extent_next, float4* copy_to,
                        const void* ctrl_src, void* ctrl_dst, size_t ctrl_bytes, hipStream_t s) {
  int nb = nblk(n, 256 * 2);  // every workgroup ends with a pair of atomics on one cache line: keep them few
  if (nb > 256) nb = 256;
  if (nb < 1) nb = 1;
  hipLaunchKernelGGL(k_time_extent, dim3(nb + (ctrl_bytes ? 1 : 0)), dim3(256), 0, s, pts, n, extent, extent_next, copy_to,
                     static_cast<const uint4*>(ctrl_src), static_cast<uint4*>(ctrl_dst), (int)(ctrl_bytes / 16));
}
void launch_sort_keys(const float4* pts, int n, unsigned int* key, unsigned int* idx, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_sort_keys, dim3(nblk(n, 256)), dim3(256), 0, s, pts, n, key, idx);
}
void launch_sort_gather(const float4* src, const unsigned int* idx, int n, float4* dst, hipStream_t s, const float* inten_src, float* inten_dst) {
  if (n <= 0) return;
  if (inten_src && inten_dst) hipLaunchKernelGGL(k_sort_gather<true>, dim3(nblk(n, 256)), dim3(256), 0, s, src, idx, n, dst, inten_src, inten_dst);
  else hipLaunchKernelGGL(k_sort_gather<false>, dim3(nblk(n, 256)), dim3(256), 0, s, src, idx, n, dst, nullptr, nullptr);
}
void launch_voxel_minmax(const float4* pts, int n, unsigned int* mm, unsigned int* mm_next, hipStream_t s) {
  int nb = nblk(n, 256 * 4);
  if (nb > 256) nb = 256;
  if (nb < 1) nb = 1;
  hipLaunchKernelGGL(k_voxel_minmax, dim3(nb), dim3(256), 0, s, pts, n, mm, mm_next);
}
void launch_voxel_keys(const float4* pts, int n, const unsigned int* mm, const unsigned int* bbox_rows, int n_rows, float leaf,
                       unsigned long long* keys, unsigned int* pcl_keys, int* filtered_dev,
                       unsigned long long* samples, int sample_width, hipStream_t s) {
  if (n > 0)
    hipLaunchKernelGGL(k_voxel_keys, dim3(nblk(n, 256)), dim3(256), 0, s, pts, n, mm, bbox_rows, n_rows, leaf, keys, pcl_keys,
                       filtered_dev, samples, sample_width);
}
// fused: the table is keyed by absolute voxel coordinates (the only form a job can share by voxel)
static VhTable vh_table(const VoxelHashBuffers* vh, int n, bool fused) {
  VhTable tb;
  memset(&tb, 0, sizeof(tb));
  if (!vh) return tb;
  tb.slots = static_cast<VhSlot*>(vh->slots);
  tb.mask = (unsigned int)voxel_hash_slots(n) - 1u;
  tb.slot_of = vh->slot_of; tb.next = vh->next; tb.crowded = vh->crowded;
  if (fused && vh->part_world > 1) {
    tb.part_world = (unsigned int)vh->part_world; tb.part_rank = (unsigned int)vh->part_rank;
    tb.part_bound = voxel_partition_bound(n, vh->part_world); tb.part_overflow = vh->part_overflow;
  }
  return tb;
}
int voxel_partition_bound(int n, int world) {
  if (world <= 1) return n;
  const long long b = (long long)n / world + (long long)n / (4 * world) + 2048;  // the mean share + 25 % + 2048: tens of standard deviations of a hashed split
  return (int)(b < n ? b : n);
}
static DeskewIo deskew_io(const DeskewPlan& p) {
  DeskewIo io;
  io.in = p.in; io.out = p.out; io.n = p.n; io.sorted = p.sorted; io.extent = p.extent; io.bbox_rows = p.bbox_rows;
  io.leaf = p.leaf;
  io.tb = vh_table(p.vh, p.n, true);
  io.ctrl_src = static_cast<const uint4*>(p.ctrl_src); io.ctrl_dst = static_cast<uint4*>(p.ctrl_dst); io.ctrl_vec = (int)(p.ctrl_bytes / 16);
#ifdef LII_GAP_TRACE
  io.gap = p.gap;
#endif
  return io;
}
template <bool FUSE, int KP>
static void launch_deskew_imu_t(const DeskewIo& io, const UndistArg& u, int K, const double* poses_host, const double* poses_dev, int nb, hipStream_t s) {
  PoseTab<KP> tab;
  if (KP > 0) memcpy(tab.v, poses_host, sizeof(double) * 22 * (size_t)K);
  hipLaunchKernelGGL((k_deskew_imu<FUSE, KP>), dim3(nb), dim3(256), 0, s, io, u, K, poses_dev, tab);
}
// poses_host != nullptr and K <= 64: the table travels in the kernel arguments; otherwise it is read from poses_dev.
// p.vh != nullptr (and p.leaf > 0): the insert of the hashed voxel filter rides along (launch_voxel_hash(..., stages = 4) goes on).
void launch_deskew_imu(const DeskewPlan& p, const double* poses_host, const double* poses_dev, int K, const UndistArgH& uh, hipStream_t s) {
  if (p.n <= 0) return;
  UndistArg u;
  static_assert(sizeof(UndistArg) == sizeof(UndistArgH), "layout");
  memcpy(&u, &uh, sizeof(u));
  const DeskewIo io = deskew_io(p);
  const int nb = nblk(p.n, 256) + (io.ctrl_vec > 0 ? 1 : 0);
  const bool fuse = p.vh != nullptr;
  const int kp = !poses_host ? 0 : (K <= 16 ? 16 : (K <= 32 ? 32 : (K <= 64 ? 64 : 0)));
  if (fuse) {
    if (kp == 16) launch_deskew_imu_t<true, 16>(io, u, K, poses_host, poses_dev, nb, s);
    else if (kp == 32) launch_deskew_imu_t<true, 32>(io, u, K, poses_host, poses_dev, nb, s);
    else if (kp == 64) launch_deskew_imu_t<true, 64>(io, u, K, poses_host, poses_dev, nb, s);
    else launch_deskew_imu_t<true, 0>(io, u, K, poses_host, poses_dev, nb, s);
  } else {
    if (kp == 16) launch_deskew_imu_t<false, 16>(io, u, K, poses_host, poses_dev, nb, s);
    else if (kp == 32) launch_deskew_imu_t<false, 32>(io, u, K, poses_host, poses_dev, nb, s);
    else if (kp == 64) launch_deskew_imu_t<false, 64>(io, u, K, poses_host, poses_dev, nb, s);
    else launch_deskew_imu_t<false, 0>(io, u, K, poses_host, poses_dev, nb, s);
  }
}
void launch_deskew_imu_dev(const DeskewPlan& p, const double* pose24_dev, const int* n_poses_dev, const double* poses_dev, hipStream_t s) {
  if (p.n <= 0) return;
  DeskewIo io = deskew_io(p);
  io.ctrl_vec = 0;  // (k_imu_propagate has pulled the control block)
  const int nb = nblk(p.n, 256);
  const UndistArg* u = reinterpret_cast<const UndistArg*>(pose24_dev);
  if (p.vh) hipLaunchKernelGGL(k_deskew_imu_dev<true>, dim3(nb), dim3(256), 0, s, io, u, n_poses_dev, poses_dev);
  else hipLaunchKernelGGL(k_deskew_imu_dev<false>, dim3(nb), dim3(256), 0, s, io, u, n_poses_dev, poses_dev);
}
void launch_deskew_imu_gated(const DeskewPlan& p, const DeskewGate& gate, hipStream_t s) {
  if (p.n <= 0) return;
  const DeskewIo io = deskew_io(p);
  const int nb = nblk(p.n, 256) + 1;  // (+ the gate workgroup, which also pulls the control block)
  if (p.vh) hipLaunchKernelGGL(k_deskew_imu_gated<true>, dim3(nb), dim3(256), 0, s, io, gate);
  else hipLaunchKernelGGL(k_deskew_imu_gated<false>, dim3(nb), dim3(256), 0, s, io, gate);
}
void launch_deskew_cv(const DeskewPlan& p, const CvArgH& ah, hipStream_t s) {
  if (p.n <= 0) return;
  CvArg a;
  static_assert(sizeof(CvArg) == sizeof(CvArgH), "layout");
  memcpy(&a, &ah, sizeof(a));
  const DeskewIo io = deskew_io(p);
  const int nb = nblk(p.n, 256) + (io.ctrl_vec > 0 ? 1 : 0);
  if (p.vh) hipLaunchKernelGGL(k_deskew_cv<true>, dim3(nb), dim3(256), 0, s, io, a);
  else hipLaunchKernelGGL(k_deskew_cv<false>, dim3(nb), dim3(256), 0, s, io, a);
}
void launch_deskew_cv_prop(const DeskewPlan& p, const CvFuseH& fh, hipStream_t s) {
  if (p.n <= 0) return;
  CvFuseArg f;
  static_assert(sizeof(CvFuseArg) == sizeof(CvFuseH), "layout");
  memcpy(&f, &fh, sizeof(f));
  const DeskewIo io = deskew_io(p);
  const int nb = nblk(p.n, 256) + 1;  // (+ the workgroup that propagates)
  if (p.vh) hipLaunchKernelGGL(k_deskew_cv_prop<true>, dim3(nb), dim3(256), 0, s, io, f);
  else hipLaunchKernelGGL(k_deskew_cv_prop<false>, dim3(nb), dim3(256), 0, s, io, f);
}
void launch_voxel_hash_clear(const VoxelHashBuffers& vh, size_t slots, hipStream_t s) {
  hipLaunchKernelGGL(k_vh_clear, dim3((unsigned int)((slots + 255) / 256)), dim3(256), 0, s, static_cast<VhSlot*>(vh.slots), (unsigned int)slots);
}
// stages: 1 = insert keyed by the PCL voxel index (stand-alone filter), 2 = its emit, 4 = the emit behind a fused de-skew
// (the table is keyed by absolute voxel coordinates).  epoch: the number of this filter run (never 0; VoxelHashBuffers::counts).
void launch_voxel_hash(const VoxelHashBuffers& vh, const float4* pts, int n, const unsigned int* mm, const unsigned int* bbox_rows,
                       int n_rows, float leaf, float4* out, int* n_out, int* filtered, unsigned int* pcl_out, int stages, unsigned int epoch,
                       hipStream_t s, int test_late, const float* inten, float* inten_out) {
  if (n <= 0) return;
  const bool wi = inten != nullptr && inten_out != nullptr;
  const VhTable tb = vh_table(&vh, n, (stages & 4) != 0);
  const int nb = nblk(n, 256);
  if (stages & 1) hipLaunchKernelGGL(k_vhash_insert, dim3(nb), dim3(256), 0, s, pts, n, mm, bbox_rows, n_rows, leaf, tb, filtered);
  const float* const no_in = nullptr;
  float* const no_out = nullptr;
  if ((stages & 2) && !wi) hipLaunchKernelGGL((k_vhash_emit<false, false>), dim3(nb), dim3(256), 0, s, pts, n, tb, vh.counts, epoch, out, n_out, pcl_out, nullptr, 0, leaf, filtered, test_late, no_in, no_out);
  if ((stages & 2) && wi) hipLaunchKernelGGL((k_vhash_emit<false, true>), dim3(nb), dim3(256), 0, s, pts, n, tb, vh.counts, epoch, out, n_out, pcl_out, nullptr, 0, leaf, filtered, test_late, inten, inten_out);
  if ((stages & 4) && !wi) hipLaunchKernelGGL((k_vhash_emit<true, false>), dim3(nb), dim3(256), 0, s, pts, n, tb, vh.counts, epoch, out, n_out, pcl_out, bbox_rows, n_rows, leaf, filtered, test_late, no_in, no_out);
  if ((stages & 4) && wi) hipLaunchKernelGGL((k_vhash_emit<true, true>), dim3(nb), dim3(256), 0, s, pts, n, tb, vh.counts, epoch, out, n_out, pcl_out, bbox_rows, n_rows, leaf, filtered, test_late, inten, inten_out);
}
size_t voxel_hash_slots(int max_n) {
  size_t slots = 1024;
  while (slots < 4u * (size_t)max_n) slots <<= 1;
  return slots;
}
float ord_to_float(unsigned int o) {
  unsigned int u = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

}  // namespace lii
