// The search launch of the LI-Init hot path for gfx950 (CDNA4, wave64).  Hand-written.
//
// Kernel and the reference code it replaces (paths relative to the reference root):
//   k_knn_ck           KD_TREE::Nearest_Search (ikd_Tree.cpp:349-379, Search :825-968) for every point of the scan, after
//                      pointBodyToWorld (src/laserMapping.cpp:209-220, call :973-985): four lanes per query, chunked scan, packed keys
//   (the searches it cannot prove exact are finished by the fit launch: lii_fit.hip)
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <math.h>
#include <stdint.h>
#include <utility>

#include "lii_search.h"
#include "lii_launch.h"

namespace lii {

// ------------------------------------------------------------------------------------------------
// The search pass: LPQ (4 by default, 8 optional) lanes per query with box-distance pruning in two rounds.
// Round 1: the 2x2x2 block of cells nearest to the query (own cell + the neighbour on the nearer side of every axis) —
// exactly one cell per lane — which covers the ball of radius g0 = min_axis max(f, cs - f) >= cs / 2 around the query.
// If the merged 5th distance is within g0 the search is complete (the usual case for a converged map).
// Round 2: the other 19 cells of the 3x3x3 block, each tested against the current 5th distance first (the tree's
// calc_box_dist rule), so most of them cost neither a table lookup nor a candidate.

// NC cell lookups with their loads issued as two batches (first probes of all block-table slots, then all cell entries)
// instead of NC dependent probe -> entry chains; a probe that hits a foreign key walks on alone (load factor <= 1/8: rare).
template <int NC>
__device__ __forceinline__ void lookup_cells_batched(const GridView& g, const uint4* __restrict__ tab, const int (&ix)[NC],
                                                     const int (&iy)[NC], const int (&iz)[NC], const bool (&want)[NC],
                                                     uint2 (&out)[NC]) {
  const int bb = kCellBias >> kCoarseShift;
  if (g.win) {  // (uniform) the dense window: one load per cell; the rare cell outside the box takes the tables' way alone
    unsigned int wi[NC];
    bool in[NC];
#pragma unroll
    for (int t = 0; t < NC; t++) {
      const unsigned int ux = (unsigned)(ix[t] - g.wx0), uy = (unsigned)(iy[t] - g.wy0), uz = (unsigned)(iz[t] - g.wz0);
      in[t] = ux < (unsigned)g.wnx && uy < (unsigned)g.wny && uz < (unsigned)g.wnz;
      wi[t] = in[t] ? (uz * (unsigned)g.wny + uy) * (unsigned)g.wnx + ux : 0u;
    }
#pragma unroll
    for (int t = 0; t < NC; t++) out[t] = (want[t] && in[t]) ? g.win[wi[t]] : make_uint2(0u, 0u);
    // (a cell outside the box is EMPTY: the window covers every block the map has - and a block of margin - and is only handed to a
    // launch while the map is as the window found it.  The first form walked the block table for such a cell: the queries of a scan
    // that looks past the map's edge paid a dependent probe each for a block that cannot exist.)
    return;
  }
  unsigned long long bk[NC];
  unsigned int sl[NC];
  uint4 e[NC];
#pragma unroll
  for (int t = 0; t < NC; t++) {
    const int bx = (ix[t] >> kCoarseShift) + bb, by = (iy[t] >> kCoarseShift) + bb, bz = (iz[t] >> kCoarseShift) + bb;
    bk[t] = pack_block(bx, by, bz);
    sl[t] = hash_block(bx, by, bz) & g.block_mask;
  }
#pragma unroll
  for (int t = 0; t < NC; t++) e[t] = want[t] ? tab[sl[t]] : make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u);
  unsigned int ci[NC];
  bool hit[NC];
#pragma unroll
  for (int t = 0; t < NC; t++) {
    unsigned long long ek = ((unsigned long long)e[t].y << 32) | e[t].x;
    while (want[t] && ek != bk[t] && ek != kEmptyKey) {
      sl[t] = (sl[t] + 1) & g.block_mask;
      e[t] = tab[sl[t]];
      ek = ((unsigned long long)e[t].y << 32) | e[t].x;
    }
    hit[t] = want[t] && ek == bk[t];
    // (local_cell of lii_grid.h written out: through the helper the compiler orders the three ORs differently)
    ci[t] = e[t].z * (unsigned)kBlockCells + ((((unsigned)iz[t] & 7u) << 6) | (((unsigned)iy[t] & 7u) << 3) | ((unsigned)ix[t] & 7u));
  }
#pragma unroll
  for (int t = 0; t < NC; t++) out[t] = hit[t] ? g.cells[ci[t]] : make_uint2(0u, 0u);
}

// ------------------------------------------------------------------------------------------------
// The search pass.  Four lanes per query (16 queries per wavefront).  Geometry of both kernels below:
// Round 1: the 2x2x2 block of cells nearest to the query (own cell + the neighbour on the nearer side of every axis), two
// cells per lane, which covers the ball of radius g0 = min_axis max(f, cs - f) >= cs / 2 around the query.  If the 5th
// distance is within g0 the search is complete.
// Round 2 (only the queries that need it): the other 19 cells of the 3x3x3 block, each tested against the current 5th
// distance first (the tree's calc_box_dist rule, ikd_Tree.cpp:1279-1289).
// A query whose 3x3x3 block cannot prove its list complete is flagged (kNeedy) and finished by k_fit_reduce / k_knn_complete.

// element t of a PoseArg seen as 24 doubles, without dynamic indexing (which would push the struct into scratch memory)
__device__ __forceinline__ double pose_element(const PoseArg& ps, int t) {
  double v = 0;
#pragma unroll
  for (int e = 0; e < 9; e++) { v = t == e ? ps.R[e] : v; v = t == 12 + e ? ps.RLI[e] : v; }
#pragma unroll
  for (int e = 0; e < 3; e++) { v = t == 9 + e ? ps.p[e] : v; v = t == 21 + e ? ps.TLI[e] : v; }
  return v;
}

// Where a query sits in the grid: its cell, the nearer-side neighbour on every axis, the radius round 1 covers (g0) and the
// radius the whole 3x3x3 block covers (guard).
struct QueryCell {
  int cx, cy, cz, ox, oy, oz;
  float eps, g0, guard;
};
__device__ __forceinline__ QueryCell query_cell(const GridView& g, float wx, float wy, float wz) {
  QueryCell q;
  const float cs = g.cs;
  q.eps = 1e-6f * (fabsf(wx) + fabsf(wy) + fabsf(wz) + 8.f);
  q.cx = cell_of(wx, g.inv_cs); q.cy = cell_of(wy, g.inv_cs); q.cz = cell_of(wz, g.inv_cs);
  const float fx = fminf(fmaxf(wx - (float)q.cx * cs, 0.f), cs), fy = fminf(fmaxf(wy - (float)q.cy * cs, 0.f), cs),
              fz = fminf(fmaxf(wz - (float)q.cz * cs, 0.f), cs);
  q.ox = fx < 0.5f * cs ? -1 : 1; q.oy = fy < 0.5f * cs ? -1 : 1; q.oz = fz < 0.5f * cs ? -1 : 1;
  q.g0 = fminf(fminf(fmaxf(fx, cs - fx), fmaxf(fy, cs - fy)), fmaxf(fz, cs - fz)) - 2.f * q.eps;
  const float mfrac = fmaxf(fminf(fminf(fminf(fx, cs - fx), fminf(fy, cs - fy)), fminf(fz, cs - fz)), 0.f);
  q.guard = cs + mfrac - 2.f * q.eps;
  return q;
}

// ---- packed keys ---------------------------------------------------------------------------------
// The search pass ranks its candidates as 32-bit keys: the float bits of d2 with the low position bits (CkGeom::kPosBits: 8 with
// four lanes per query) replaced by the candidate's position in the group's candidate list - its chunk in the group's table and the
// lane that measured it.  d2 >= 0, so the keys order like the distances (to 15 mantissa bits) and are unique; a sorted list of the
// SEVEN smallest keys is maintained with one v_min_u32 and six v_med3_u32 per candidate - no compares, no selects, no index
// registers.  The lists of a group's lanes are joined by bitonic merges over DPP quad permutes.  At the end the seven winners
// are re-measured exactly and ranked exactly (distance, then position - the visiting order): the five nearest are the exact
// answer unless the exact 5th distance reaches the truncated distance of the 7th key - every candidate that was dropped is at
// least that far - in which case the query is flagged for the completion pass (5th, 6th and 7th distances equal in their kept bits:
// never observed on the bench streams).
constexpr unsigned int kPkInf = 0xFFFFFFFFu;

struct Pk7 {
  unsigned int k0, k1, k2, k3, k4, k5, k6;
};
__device__ __forceinline__ unsigned int umed3(unsigned int a, unsigned int b, unsigned int c) {
  unsigned int r;
  asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ __forceinline__ void pk_insert(Pk7& L, unsigned int x) {
  L.k6 = umed3(L.k5, L.k6, x);
  L.k5 = umed3(L.k4, L.k5, x);
  L.k4 = umed3(L.k3, L.k4, x);
  L.k3 = umed3(L.k2, L.k3, x);
  L.k2 = umed3(L.k1, L.k2, x);
  L.k1 = umed3(L.k0, L.k1, x);
  L.k0 = min(L.k0, x);
}
template <int CTRL>
__device__ __forceinline__ unsigned int quad_perm(unsigned int v) {
  return (unsigned int)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xF, 0xF, true);
}
template <int CTRL>
__device__ __forceinline__ float quad_perm_f(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, true));
}
#define LII_CE(a, b) { const unsigned int lo_ = min(a, b), hi_ = max(a, b); a = lo_; b = hi_; }
// L <- the seven smallest keys of L and of the partner lane's list (quad permute CTRL), sorted.  C_i = min(L_i, M_{7-i}) with an
// eighth "infinite" key on both sides is a bitonic sequence holding the eight smallest of the sixteen; three half-cleaner stages
// sort it.  Both partners compute the same list.
template <int CTRL>
__device__ __forceinline__ void pk_merge(Pk7& L) {
  const unsigned int m0 = quad_perm<CTRL>(L.k0), m1 = quad_perm<CTRL>(L.k1), m2 = quad_perm<CTRL>(L.k2), m3 = quad_perm<CTRL>(L.k3),
                     m4 = quad_perm<CTRL>(L.k4), m5 = quad_perm<CTRL>(L.k5), m6 = quad_perm<CTRL>(L.k6);
  unsigned int c0 = L.k0, c1 = min(L.k1, m6), c2 = min(L.k2, m5), c3 = min(L.k3, m4), c4 = min(L.k4, m3), c5 = min(L.k5, m2),
               c6 = min(L.k6, m1), c7 = m0;
  LII_CE(c0, c4) LII_CE(c1, c5) LII_CE(c2, c6) LII_CE(c3, c7)
  LII_CE(c0, c2) LII_CE(c1, c3) LII_CE(c4, c6) LII_CE(c5, c7)
  LII_CE(c0, c1) LII_CE(c2, c3) LII_CE(c4, c5)
  c6 = min(c6, c7);
  L.k0 = c0; L.k1 = c1; L.k2 = c2; L.k3 = c3; L.k4 = c4; L.k5 = c5; L.k6 = c6;
}
#undef LII_CE

template <int LPQ>
__device__ __forceinline__ void pk_group_merge(Pk7& L) {
  if (LPQ >= 2) pk_merge<0xB1>(L);  // lanes 0<->1, 2<->3
  if (LPQ == 4) pk_merge<0x4E>(L);  // lanes 0<->2, 1<->3: every lane of the group now holds the group's seven smallest keys
}
// the value lane J of the group holds
template <int LPQ, int J>
__device__ __forceinline__ float group_bcast_f(float v) {
  if (LPQ == 4) return quad_perm_f<J * 0x55>(v);
  if (LPQ == 2) return quad_perm_f<J == 0 ? 0xA0 : 0xF5>(v);
  return v;
}
// Loops whose index must be a constant expression (register arrays must never be indexed dynamically: they would move to
// scratch memory): f(std::integral_constant<int, 0>) ... f(std::integral_constant<int, N - 1>).
template <class F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}
template <class T>
__device__ __forceinline__ T by_value(T x) { return x; }
// arr[BASE + sub] for sub < LPQ as a chain of selects over constant indices (entries behind the array: the last one)
template <int LPQ, int BASE, int N, class T>
__device__ __forceinline__ T pick_by_lane(const T (&arr)[N], int sub) {
  T v = by_value(arr[BASE < N ? BASE : N - 1]);
  static_for<LPQ - 1>([&](auto jc) {
    constexpr int j = decltype(jc)::value + 1;
    v = sub == j ? by_value(arr[BASE + j < N ? BASE + j : N - 1]) : v;
  });
  return v;
}

// ---- the search pass with the GROUP scanning every cell together ("chunked", round 5) ------------------------------------------
// Rounds 3 - 4 (k_knn_pk) gave every lane of a query its own cells: a candidate load of a wavefront then touches up to 64 different cache lines -
// measured 40 per instruction (TCP_TOTAL_CACHE_ACCESSES / SQ_INSTS_VMEM_RD), 6.6 M (100 k-point scan) and 21 M (500 k) line lookups
// per launch: at one lookup per cycle and compute unit 10.7 and 34.3 us of the vector-memory front end, in launches of 17 - 21 and
// 52 - 64 us (profiles/r05_knn_l1.md).  Here the LPQ lanes of a query read LPQ CONSECUTIVE points of one cell - 64 contiguous bytes
// with four lanes, one or two lines - and neighbouring queries that scan the same cell read the same lines.
// The cells' ranges are cut into chunks of LPQ points; the group keeps a table of its chunks in LDS - word = first map index << 3 |
// points in the chunk (1 .. LPQ; 0: padding behind the last chunk, so that a batch of NB loads needs no bounds test) - in the order
// the cells were looked up: round 1's eight cells, then the outer cells round 2 adds.  A candidate is numbered (chunk << log2 LPQ) |
// lane: the position in its key.  Whatever needs a candidate's map index afterwards - the winners' re-measurement - reads it from
// the table; the per-lane range arithmetic of rounds 3 - 4 (which range does position p belong to?) is gone.
template <int LPQ>
struct CkGeom {
  static constexpr int kLaneShift = LPQ == 4 ? 2 : (LPQ == 2 ? 1 : 0);
  static constexpr int kChunkBits = 6;
  static constexpr int MAXCH = 1 << kChunkBits;                 // chunks a group can number: 64 x LPQ candidates
  static constexpr int kPosBits = kChunkBits + kLaneShift;      // 8 of the 23 mantissa bits with four lanes (rounds 3 - 4: 12)
  static constexpr unsigned int kPosMask = (1u << kPosBits) - 1u;
  static constexpr int NR = 8 / LPQ;                            // cells per lane in round 1
  static constexpr int NW = (7 + LPQ - 1) / LPQ;                // winners a lane re-measures
  static constexpr int MAXPASS = (19 + 2 * LPQ - 1) / (2 * LPQ);  // round 2: two outer cells per lane and pass
};
// sum of `v` over the lanes of the group below this one (exclusive prefix) and over all of them
template <int LPQ>
__device__ __forceinline__ void group_prefix(unsigned int v, int sub, unsigned int& before, unsigned int& total) {
  if (LPQ == 4) {
    const unsigned int v0 = quad_perm<0x00>(v), v1 = quad_perm<0x55>(v), v2 = quad_perm<0xAA>(v), v3 = quad_perm<0xFF>(v);
    before = sub == 0 ? 0u : (sub == 1 ? v0 : (sub == 2 ? v0 + v1 : v0 + v1 + v2));
    total = v0 + v1 + v2 + v3;
  } else if (LPQ == 2) {
    const unsigned int v0 = quad_perm<0xA0>(v), v1 = quad_perm<0xF5>(v);
    before = sub == 0 ? 0u : v0;
    total = v0 + v1;
  } else {
    before = 0u;
    total = v;
  }
}
// The lane's NC cell ranges become chunks at tab[at ...] (the group's table; `at` = where this lane's chunks start); the caller
// has checked that they fit.
template <int LPQ, int NC>
__device__ __forceinline__ void ck_write_chunks(unsigned int* __restrict__ tab, unsigned int at, const uint2 (&r)[NC]) {
#pragma unroll
  for (int t = 0; t < NC; t++) {
    for (unsigned int j = r[t].x; j < r[t].y; j += LPQ) tab[at++] = (j << 3) | min((unsigned)LPQ, r[t].y - j);
  }
}
// chunks [first, end) of the group's table (end is followed by >= NB - 1 padding words), NB loads in flight per lane
template <int LPQ, int NB>
__device__ __forceinline__ void ck_scan(const float4* __restrict__ pts, const unsigned int* __restrict__ tab, unsigned int first, unsigned int end,
                                        int sub, float wx, float wy, float wz, Pk7& L) {
  using G = CkGeom<LPQ>;
  for (unsigned int base = first; base < end; base += NB) {
    unsigned int w[NB];
#pragma unroll
    for (int u = 0; u < NB; u++) w[u] = tab[base + u];
    F3 P[NB];
#pragma unroll
    for (int u = 0; u < NB; u++) P[u] = load_xyz(pts, (w[u] >> 3) + min((unsigned)sub, (w[u] & 7u) - 1u));  // (padding: count 0 -> slot `sub` of the array, discarded)
#pragma unroll
    for (int u = 0; u < NB; u++) {
      const float d = dist2_ref(wx, wy, wz, P[u].x, P[u].y, P[u].z);
      const unsigned int key = (__float_as_uint(d) & ~G::kPosMask) | (((base + u) << G::kLaneShift) | (unsigned)sub);
      pk_insert(L, (unsigned)sub < (w[u] & 7u) ? key : kPkInf);  // (the acceptance test d2 <= max_d2 waits for the re-measurement of the winners)
    }
  }
}
// `forced` > 0: always runs (a host-driven pass: the host has put the pose into `pose`, device memory).
// forced < 0: device-driven loop — pose from `pose` (the control block), runs only when the control block says the next pass
// searches and the loop has not stopped (src/laserMapping.cpp:978, :1102-1106).  An executed pass leaves its pose in
// `search_pose_out` (may be null).
// LPQ = lanes per query (4; 2 lanes issue fewer instructions in total but lose to latency and to the vector-memory front end at every
// size measured: profiles/r05_knn_lpq.md); NB = candidate loads a lane keeps in flight (one batch).
template <int LPQ, int BS, int NB, int WPE>
__global__ __launch_bounds__(BS, WPE) void k_knn_ck(GridView g, RegistrationBuffers rb, const PoseArg* __restrict__ pose,
                                               const IekfCtrl* __restrict__ ctrl, int forced, int nb_real,
                                               double* __restrict__ search_pose_out, int epoch) {
  using G = CkGeom<LPQ>;
  constexpr int QPB = BS / LPQ;
  __shared__ unsigned int s_tab[QPB * (G::MAXCH + NB)];
  // Everything the head of the kernel needs from memory is requested AT ONCE, before anything is waited for: the query point itself
  // (an unsharded cloud: its index depends on nothing that has to be loaded; index clamped, a lane beyond the cloud discards it) and -
  // load_head_scalars - the pose, the loop flags and the size of the cloud.  Round 4 had the flags behind the size behind the pose
  // (24 dependent scalar loads) and the point behind all of them.
  const int blk = xcd_remap(blockIdx.x, nb_real);
  const int sub = threadIdx.x & (LPQ - 1);
  const int ql = blk * QPB + (int)(threadIdx.x / LPQ);
  const bool early = rb.shard_world <= 1;
  float4 pb_early = make_float4(0.f, 0.f, 0.f, 0.f);
  if (early) pb_early = rb.body[min(max(ql, 0), rb.cap - 1)];
  const HeadScalars hs = load_head_scalars(pose, &ctrl->search_next, rb.n_dev ? rb.n_dev : &ctrl->max_it, &ctrl->max_it);
  const PoseArg& ps = hs.ps;
  const int c_search = hs.search_next, c_stop = hs.stop, n_mem = hs.n_mem;
  int lo, n_live;
  shard_range_n(rb, n_mem, lo, n_live);
  // (the list of unfinished queries: launch number e appends to slot e & 1; EVERY enqueued launch - whether its pass is due or not -
  // empties the other slot for launch e + 1: its readers, the fit launch behind launch e - 1, are done)
  if (epoch > 0 && blockIdx.x == 0 && threadIdx.x == 0) rb.flag_count[(epoch + 1) & 1] = 0;
  if (forced < 0 && (c_stop || !c_search)) return;
  if (search_pose_out && blockIdx.x == 0 && threadIdx.x < 24) search_pose_out[threadIdx.x] = pose_element(ps, threadIdx.x);
  if (blk >= nb_real) return;
  if (blk * QPB + (int)((threadIdx.x & ~63u) / LPQ) >= n_live) return;
  const int qi = lo + ql;
  const bool live = ql < n_live;
  float wx = 0, wy = 0, wz = 0;
  if (live && sub == 0) body_to_world(ps, early ? pb_early : rb.body[qi], wx, wy, wz);
  wx = group_bcast_f<LPQ, 0>(wx); wy = group_bcast_f<LPQ, 0>(wy); wz = group_bcast_f<LPQ, 0>(wz);
  const bool active = live && g.n_pts > 0;
  const float INF = __builtin_inff();
  const uint4* __restrict__ tab_blocks = reinterpret_cast<const uint4*>(g.blocks);
  const float4* __restrict__ pts = g.pts;
  unsigned int* const tab = s_tab + (threadIdx.x / LPQ) * (G::MAXCH + NB);

  // Round 1: the 2x2x2 block of cells nearest to the query, NR cells per lane (looked up as a batch), their chunks into the table
  const QueryCell q = query_cell(g, wx, wy, wz);
  const float g0sq = q.g0 * q.g0, guardsq = q.guard * q.guard;
  unsigned int n_chunks;  // chunks in the group's table (group-uniform)
  bool ovf;
  {
    uint2 r[G::NR];
    int jx[G::NR], jy[G::NR], jz[G::NR];
    bool want[G::NR];
#pragma unroll
    for (int t = 0; t < G::NR; t++) {
      const int c = sub * G::NR + t;
      jx[t] = q.cx + ((c & 1) ? q.ox : 0); jy[t] = q.cy + ((c & 2) ? q.oy : 0); jz[t] = q.cz + ((c & 4) ? q.oz : 0);
      want[t] = true;
    }
    lookup_cells_batched<G::NR>(g, tab_blocks, jx, jy, jz, want, r);
    unsigned int mine = 0u;
#pragma unroll
    for (int t = 0; t < G::NR; t++) {
      if (!active) r[t] = make_uint2(0u, 0u);
      mine += (r[t].y - r[t].x + (unsigned)LPQ - 1u) / (unsigned)LPQ;
    }
    unsigned int before;
    group_prefix<LPQ>(mine, sub, before, n_chunks);
    // a group whose cells hold more than MAXCH x LPQ points is left to the completion pass (cells of hundreds of points)
    ovf = n_chunks > (unsigned)G::MAXCH;
    if (ovf) n_chunks = 0u;
    else ck_write_chunks<LPQ, G::NR>(tab, before, r);
    if (sub == 0) {
#pragma unroll
      for (int u = 0; u < NB - 1; u++) tab[n_chunks + u] = 0u;  // padding: a batch of loads runs past the last chunk
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const bool fast = active && !ovf;
  Pk7 L;
  L.k0 = L.k1 = L.k2 = L.k3 = L.k4 = L.k5 = L.k6 = kPkInf;
  ck_scan<LPQ, NB>(pts, tab, 0u, n_chunks, sub, wx, wy, wz, L);
  pk_group_merge<LPQ>(L);

  // Round 2 (the tree's calc_box_dist rule, ikd_Tree.cpp:1279-1289): is the 5th distance - here its upper bound, the 5th key with the
  // position bits set - within the radius round 1 covers?  If not, the outer cells of the 3x3x3 block that can
  // still hold a closer point, two per lane and pass; their chunks continue the table.
  {
    const float ub5 = L.k4 != kPkInf ? __uint_as_float(L.k4 | G::kPosMask) : INF;
    const float bound = fminf(ub5, g.max_d2);
    const bool need2 = fast && !(bound <= g0sq);
    if (__any(need2)) {
      float GX[3], GY[3], GZ[3];
      {
        const float nx = axis_gap(wx, q.cx + q.ox, g.cs, q.eps), fx = axis_gap(wx, q.cx - q.ox, g.cs, q.eps);
        const float ny = axis_gap(wy, q.cy + q.oy, g.cs, q.eps), fy = axis_gap(wy, q.cy - q.oy, g.cs, q.eps);
        const float nz = axis_gap(wz, q.cz + q.oz, g.cs, q.eps), fz = axis_gap(wz, q.cz - q.oz, g.cs, q.eps);
        GX[0] = 0.f; GX[1] = nx * nx; GX[2] = fx * fx;
        GY[0] = 0.f; GY[1] = ny * ny; GY[2] = fy * fy;
        GZ[0] = 0.f; GZ[1] = nz * nz; GZ[2] = fz * fz;
      }
      unsigned int m = 0u;
      static_for<27>([&](auto cc) {
        constexpr int c = decltype(cc)::value, sx = c % 3, sy = (c / 3) % 3, sz = c / 9;
        if constexpr (sx == 2 || sy == 2 || sz == 2) {
          const float d = GX[sx] + GY[sy] + GZ[sz];
          m |= d > bound ? 0u : (1u << c);
        }
      });
      m = need2 ? m : 0u;
      // the group's list continues on lane 0 alone (copies would come back as duplicates), the other lanes start empty
      if (sub != 0) L.k0 = L.k1 = L.k2 = L.k3 = L.k4 = L.k5 = L.k6 = kPkInf;
      unsigned int t = m;
#pragma unroll
      for (int j = 0; j < LPQ - 1; j++) t = j < sub ? (t & (t - 1u)) : t;  // the lane's first survivor: number `sub` of the set bits
      for (int pass = 0; pass < G::MAXPASS; pass++) {
        if (!__any(t != 0u)) break;
        const int c1 = t ? __ffs((int)t) - 1 : -1;
#pragma unroll
        for (int j = 0; j < LPQ; j++) t = t & (t - 1u);
        const int c2 = t ? __ffs((int)t) - 1 : -1;
#pragma unroll
        for (int j = 0; j < LPQ; j++) t = t & (t - 1u);
        uint2 r[2];
        {
          int jx[2], jy[2], jz[2];
          const bool want[2] = {true, true};
          const int ca = c1 < 0 ? 0 : c1, cb = c2 < 0 ? 0 : c2;  // (0 = the query's own cell: looked up for nothing, not branched around)
          auto step = [](int sdig, int o) { return o * ((sdig & 1) - (sdig >> 1)); };
          jx[0] = q.cx + step(ca % 3, q.ox); jy[0] = q.cy + step((ca / 3) % 3, q.oy); jz[0] = q.cz + step(ca / 9, q.oz);
          jx[1] = q.cx + step(cb % 3, q.ox); jy[1] = q.cy + step((cb / 3) % 3, q.oy); jz[1] = q.cz + step(cb / 9, q.oz);
          lookup_cells_batched<2>(g, tab_blocks, jx, jy, jz, want, r);
        }
        if (c1 < 0) r[0] = make_uint2(0u, 0u);
        if (c2 < 0) r[1] = make_uint2(0u, 0u);
        const unsigned int mine = (r[0].y - r[0].x + (unsigned)LPQ - 1u) / (unsigned)LPQ + (r[1].y - r[1].x + (unsigned)LPQ - 1u) / (unsigned)LPQ;
        unsigned int before, add;
        group_prefix<LPQ>(mine, sub, before, add);
        const unsigned int from = n_chunks;
        if (from + add > (unsigned)G::MAXCH) {  // out of table: the group stops here and is left to the completion pass
          ovf = true;
          t = 0u;
          add = 0u;
        } else {
          ck_write_chunks<LPQ, 2>(tab, from + before, r);
        }
        n_chunks = from + add;
        if (sub == 0) {
#pragma unroll
          for (int u = 0; u < NB - 1; u++) tab[n_chunks + u] = 0u;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        ck_scan<LPQ, NB>(pts, tab, from, n_chunks, sub, wx, wy, wz, L);
      }
      pk_group_merge<LPQ>(L);
    }
  }

  // Exact re-measurement of the seven winners: a key's position names its chunk and lane, the table gives the map index - lane `sub`
  // loads and measures winners sub, sub + LPQ, ..., and the seven exact distances are shared by broadcasts inside the group.
  float e[7];
  F3 W[G::NW];
  float d7t;
  bool tie = false;
  {
    const unsigned int K[7] = {L.k0, L.k1, L.k2, L.k3, L.k4, L.k5, L.k6};
    float el[G::NW];
    static_for<G::NW>([&](auto ic) {
      constexpr int i = decltype(ic)::value;
      const unsigned int key = pick_by_lane<LPQ, LPQ * i>(K, sub);
      const unsigned int pos = key == kPkInf ? 0u : (key & G::kPosMask);  // (an empty slot reads chunk 0 - or padding - and is discarded)
      W[i] = load_xyz(pts, (tab[pos >> G::kLaneShift] >> 3) + (pos & (unsigned)(LPQ - 1)));
    });
#pragma unroll
    for (int w = 0; w < 6; w++) tie = tie || ((K[w] ^ K[w + 1]) <= G::kPosMask && K[w + 1] != kPkInf);
    d7t = K[6] != kPkInf ? __uint_as_float(K[6] & ~G::kPosMask) : INF;
#pragma unroll
    for (int i = 0; i < G::NW; i++) el[i] = dist2_ref(wx, wy, wz, W[i].x, W[i].y, W[i].z);
    e[0] = group_bcast_f<LPQ, 0 % LPQ>(el[0 / LPQ]); e[1] = group_bcast_f<LPQ, 1 % LPQ>(el[1 / LPQ]);
    e[2] = group_bcast_f<LPQ, 2 % LPQ>(el[2 / LPQ]); e[3] = group_bcast_f<LPQ, 3 % LPQ>(el[3 / LPQ]);
    e[4] = group_bcast_f<LPQ, 4 % LPQ>(el[4 / LPQ]); e[5] = group_bcast_f<LPQ, 5 % LPQ>(el[5 / LPQ]);
    e[6] = group_bcast_f<LPQ, 6 % LPQ>(el[6 / LPQ]);
#pragma unroll
    for (int w = 0; w < 7; w++) e[w] = (K[w] != kPkInf && e[w] <= g.max_d2) ? e[w] : INF;  // acceptance: d2 <= max_d2 (quirk A5)
  }
  // Exact ranks of this lane's winners and the exact 5th distance.  The keys are in ascending order, so the exact order can differ
  // from the key order only where the distance bits of neighbouring keys agree (a wavefront without such a pair skips the ranking),
  // and there an equal exact distance keeps the key order (position = visiting order).
  int rk[G::NW];
#pragma unroll
  for (int i = 0; i < G::NW; i++) rk[i] = sub + LPQ * i;
  float d5 = e[4];
  if (__any(tie)) {
    int rank[7];
#pragma unroll
    for (int w = 0; w < 7; w++) rank[w] = 0;
#pragma unroll
    for (int v = 0; v < 7; v++)
#pragma unroll
      for (int w = v + 1; w < 7; w++) {
        const bool swapped = e[v] > e[w];
        rank[w] += swapped ? 0 : 1;
        rank[v] += swapped ? 1 : 0;
      }
    d5 = INF;
#pragma unroll
    for (int w = 0; w < 7; w++) d5 = rank[w] == 4 ? e[w] : d5;
    static_for<G::NW>([&](auto ic) {
      constexpr int i = decltype(ic)::value;
      rk[i] = pick_by_lane<LPQ, LPQ * i>(rank, sub);
    });
  }
  const int found = e[4] < INF ? 5 : (e[3] < INF ? 4 : (e[2] < INF ? 3 : (e[1] < INF ? 2 : (e[0] < INF ? 1 : 0))));
  const bool amb = d7t < INF && !(d5 < d7t);
  const bool need = active && (ovf || amb || !(fminf(d5, g.max_d2) <= guardsq));
  if (live) {
    static_for<G::NW>([&](auto ic) {
      constexpr int i = decltype(ic)::value;
      const float ei = pick_by_lane<LPQ, LPQ * i>(e, sub);
      if (sub + LPQ * i < 7 && ei < INF && rk[i] < 5) rb.nbr[(size_t)rk[i] * rb.cap + qi] = make_float4(W[i].x, W[i].y, W[i].z, ei);
    });
    if (found < 5) {  // the missing neighbours read (0, 0, 0, inf)
#pragma unroll
      for (int r = 0; r < 5; r += LPQ)
        if (sub + r < 5 && sub + r >= found) rb.nbr[(size_t)(sub + r) * rb.cap + qi] = make_float4(0.f, 0.f, 0.f, INF);
    }
    if (sub == (LPQ > 1 ? 1 : 0)) {
      const int cflags = found | (need ? (kNeedy | ((ovf || amb) ? 0 : kCovered)) : 0);
      rb.nbr_count[qi] = cflags;
      if (need && epoch > 0) {  // listed for the completion workgroups of the fit launch behind this one (~80 of 95 k queries)
        const int at = atomicAdd(&rb.flag_count[epoch & 1], 1);
        if (at < kListCap) {
          float4* e = rb.flag_list + 2 * ((epoch & 1) * kListCap + at);
          e[0] = make_float4(wx, wy, wz, __int_as_float(qi));
          e[1] = make_float4(__int_as_float(cflags), 0.f, 0.f, 0.f);
        }
      }
    }
    if (sub == (LPQ == 4 ? 2 : 0)) rb.world[qi] = make_float4(wx, wy, wz, 0.f);
  }
}

static inline int nblk(int n, int b) { return (n + b - 1) / b; }
// The search launch: k_knn_ck, four lanes per query.
// 128 lanes per workgroup, 6 loads in flight per lane, 7 wavefronts per SIMD (69 VGPRs): measured on the per-lane form of rounds 3 - 4
// against 64 / 256 lanes, 4 .. 12 loads, 6 / 8 wavefronts per SIMD (within 1 - 2 %: profiles/r03_knn_ab.md), and 2 / 1 lanes per query
// (slower at every cloud size: profiles/r05_knn_lpq.md).
constexpr int kKnnBs = 128, kKnnNb = 6, kKnnWpe = 7;
// epoch: the number of this search launch (> 0; the fit launch behind it gets the same) - or 0: no list of unfinished queries, every
// workgroup of the fit launch finishes its own (the map update's repeated search)
void launch_knn(const GridView& g, const RegistrationBuffers& rb, const PoseArg* pose,
                const IekfCtrl* ctrl, int forced, double* search_pose_out, hipStream_t s, int epoch, hipEvent_t ev_start, hipEvent_t ev_stop) {
  int nq = nblk(shard_bound(rb), kKnnBs / 4);
  if (nq < 1) nq = 1;
  const int nq_pad = ((nq + 7) / 8) * 8;
  if (ev_start && ev_stop) {  // (measurement: the dispatch's own time stamps, no barrier packets around it)
    hipExtLaunchKernelGGL((k_knn_ck<4, kKnnBs, kKnnNb, kKnnWpe>), dim3(nq_pad), dim3(kKnnBs), 0, s, ev_start, ev_stop, 0u, g, rb, pose, ctrl, forced, nq,
                          search_pose_out, epoch);
    return;
  }
  hipLaunchKernelGGL((k_knn_ck<4, kKnnBs, kKnnNb, kKnnWpe>), dim3(nq_pad), dim3(kKnnBs), 0, s, g, rb, pose, ctrl, forced, nq, search_pose_out, epoch);
}
}  // namespace lii
