// libliinit_hip - the registered clouds of a scan (lii_publish_*): what laserMapping's loop hands out BEHIND the update
// (src/laserMapping.cpp:1152-1156): publish_frame_world (:561-614, with the pcl_wait_save append of :594-613), publish_effect_world
// (:625-636).  One launch: pointBodyToWorld (:209-220; body_to_world, lii_device.h - fp64 arithmetic, float result, no FMA contraction
// in this unit) at the state the stopping pass left in the control block, over the de-skewed scan and over the down-sampled cloud,
// whose selected points (laserCloudOri) are compacted in ascending index on the way.
#include "lii_launch.h"

namespace lii {
namespace {

// selected points among the 256 of down-sampled block q (every lane calls it; contains a barrier)
__device__ __forceinline__ unsigned int publish_count(bool sel, unsigned int* s_c /*[4]*/, unsigned long long* mask_out) {
  const unsigned long long m = __ballot(sel);
  if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = (unsigned int)__popcll(m);
  __syncthreads();
  *mask_out = m;
  return s_c[0] + s_c[1] + s_c[2] + s_c[3];
}

// lii_publish_wire_set: one pcl::PointXYZINormal record as three 16-byte pieces - x y z 1.0f | normal 0 0 0, pad 0 | intensity curvature 0 0
struct WireRecord { uint4 q[kWireQuads]; };
__device__ __forceinline__ WireRecord wire_record(float x, float y, float z, unsigned int intensity, unsigned int curvature) {
  WireRecord r;
  r.q[0] = make_uint4(__float_as_uint(x), __float_as_uint(y), __float_as_uint(z), 0x3F800000u);
  r.q[1] = make_uint4(0u, 0u, 0u, 0u);
  r.q[2] = make_uint4(intensity, curvature, 0u, 0u);
  return r;
}

// The records of workgroup `blk`'s first n_here points -> cloud[blk * 256 ...]: 12 288 contiguous, 16-byte-aligned bytes when the slab
// is full.  Every lane of the workgroup calls it with its record (any, where it has no point).  The records are laid out in LDS (lane t:
// pieces 3t .. 3t + 2 - ds_write_b128 at a stride of 12 dwords: the 8 lanes of a store's lane group start at banks 0 12 24 4 16 28 8 20
// of 32, four banks each: no conflict) and written back as 768 consecutive pieces, lane t storing t, t + 256, t + 512: a wave
// instruction covers 1 KiB contiguously.  Measured against each lane storing its own record at a stride of 48 bytes: 10.6 us per launch
// against 15.1 us on the stream100k shapes (profiles/publish_wire.md).
__device__ __forceinline__ void wire_store_slab(uint4* __restrict__ cloud, int blk, int n_here, const WireRecord& r) {
  uint4* out = cloud + (size_t)blk * 256 * kWireQuads;
  __shared__ uint4 s_rec[256 * kWireQuads];
  const int t = (int)threadIdx.x;
  __syncthreads();  // (the slab of the cloud before this one has been read)
  s_rec[kWireQuads * t] = r.q[0]; s_rec[kWireQuads * t + 1] = r.q[1]; s_rec[kWireQuads * t + 2] = r.q[2];
  __syncthreads();
  const int pieces = n_here * kWireQuads;
  for (int k = 0; k < kWireQuads; k++)
    if (t + 256 * k < pieces) out[t + 256 * k] = s_rec[t + 256 * k];
}

}  // namespace

// Workgroups [0, a.dense_blocks): the de-skewed scan -> a.dense (LII_PUB_DENSE) and / or behind the points of the save buffer;
// the workgroups behind them: the down-sampled cloud -> a.down (LII_PUB_DOWN) and its selected points -> a.effect (LII_PUB_EFFECT).
// guard != nullptr: the launch was enqueued behind the passes of iterated update `seq` before the host knew how it ends - the pose is
// the control block's (IekfCtrl::st leads it), and the launch does nothing unless that update has stopped regularly (the test
// k_map_decide makes): the host enqueues it again behind a loop it had to continue.
// The effect cloud's places come from an in-launch prefix of the workgroups' counts (prefix_below, lii_device.h) and wavefront
// ballots: ascending index, the same on every run - never the arrival order of a counter.
// The save buffer's append offset ping-pongs between two words (a.save_ctl[par] is read by everybody, [par ^ 1] written by one
// lane: no lane reads what another writes in this launch); a scan that does not fit writes nothing and raises a.save_ctl[2].
// LII_PUB_INTENSITY: the workgroups of the scan also hand its intensities on - to a.dense_int, and to a.save_int at the offset and under
// the fits / does-not-fit decision of the cloud's append (this launch owns the offset: one behind it would read a moved one; a scan
// without intensities appends 0.0f, the two buffers stay aligned) -, those of the down-sampled cloud a.body_int to a.down_int.  With the
// five pointers null the launch is the INT = false instantiation: the kernel without the channel, instruction for instruction.
// lii_publish_wire_set (WIRE): the same workgroups also form the clouds as 48-byte pcl::PointXYZINormal records (include/liinit_hip.h:
// x y z 1.0f | 0 0 0 0 | intensity curvature 0 0) - the scan's write the DENSE and the BODY record (curvature: 0 / t_ms), the
// down-sampled cloud's the DOWN record and, at the compacted place, the EFFECT record (intensity sqrt(1000), src/laserMapping.cpp:1050-1051;
// under lii_point_noise_set's model 1 the point's own sqrt(R_inv_i), a.w_effect_int).
// A workgroup's 256 records of DENSE / BODY / DOWN are 12 288 contiguous bytes: wire_store_slab.  With the six pointers null the launch is
// the WIRE = false instantiation: the code of the kernel without the order.
template <bool INT, bool WIRE>
__global__ __launch_bounds__(256) void k_publish_world(PublishArgs a, PoseArg ps_val) {
  const IekfCtrl* __restrict__ guard = a.guard;
  const PoseArg ps = load_pose(guard != nullptr, reinterpret_cast<const PoseArg*>(guard), ps_val);
  const bool go = !guard || (guard->stop == 1 && guard->singular == 0 && guard->seq == a.seq);  // uniform over the launch
  if ((int)blockIdx.x < a.dense_blocks) {
    int off = 0;
    bool fits = false;
    if (a.save) {
      off = a.save_ctl[a.save_par];
      fits = go && off >= 0 && (long long)off + a.n_scan <= (long long)a.save_cap;
      if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.save_ctl[a.save_par ^ 1] = fits ? off + a.n_scan : off;
        if (go && !fits) a.save_ctl[2] = 1;
      }
    }
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (WIRE ? !go : (!go || i >= a.n_scan)) return;  // (WIRE: the whole workgroup stays for wire_store_slab's barriers)
    const bool live = !WIRE || i < a.n_scan;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f), o = p;
    if (live) {
      p = a.scan[i];
      float wx, wy, wz;
      body_to_world(ps, p, wx, wy, wz);
      o = make_float4(wx, wy, wz, p.w);
      if (a.dense) a.dense[i] = o;
      if (fits) a.save[(size_t)off + i] = o;
      if (INT && (a.dense_int || a.save_int)) {
        const float q = a.scan_int ? a.scan_int[i] : 0.f;
        if (a.dense_int) a.dense_int[i] = q;
        if (fits && a.save_int) a.save_int[(size_t)off + i] = q;
      }
    }
    if (WIRE) {
      const int n_here = min(256, a.n_scan - (int)blockIdx.x * 256);
      const unsigned int q = (live && a.w_scan_int) ? __float_as_uint(a.w_scan_int[i]) : 0u;
      if (a.w_dense) wire_store_slab(a.w_dense, (int)blockIdx.x, n_here, wire_record(o.x, o.y, o.z, q, 0u));
      if (a.w_body) wire_store_slab(a.w_body, (int)blockIdx.x, n_here, wire_record(p.x, p.y, p.z, q, __float_as_uint(p.w)));
    }
    return;
  }
  if (!go) return;  // (every workgroup of the launch takes the same way: nobody waits for a word that never comes)
  const int b = (int)blockIdx.x - a.dense_blocks;
  const int n_mem = a.n_body_dev ? *a.n_body_dev : a.n_body;
  const int n = n_mem < a.n_body ? n_mem : a.n_body;  // a.n_body: the launch bound (the buffers' capacity holds it)
  const int j = b * 256 + (int)threadIdx.x;
  const bool live = j < n;
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) {
    const float4 p = a.body[j];
    float wx, wy, wz;
    body_to_world(ps, p, wx, wy, wz);
    o = make_float4(wx, wy, wz, p.w);
    if (a.down) a.down[j] = o;
    if (INT && a.down_int) a.down_int[j] = a.body_int[j];
  }
  if (WIRE && a.w_down) {
    const unsigned int q = (live && a.w_body_int) ? __float_as_uint(a.w_body_int[j]) : 0u;
    wire_store_slab(a.w_down, b, max(0, min(256, n - b * 256)), wire_record(o.x, o.y, o.z, q, 0u));
  }
  const int n_down_blocks = (int)gridDim.x - a.dense_blocks;
  if (!a.effect && !(WIRE && a.w_effect)) {
    if (b == n_down_blocks - 1 && threadIdx.x == 0) { a.counts_dev[0] = n; a.counts_dev[1] = 0; a.counts_host[0] = n; a.counts_host[1] = 0; }
    return;
  }
  __shared__ unsigned int s_c[4], s_r[4], s_sum[12];
  const bool sel = live && a.selected[j] != 0;
  unsigned long long mask;
  const unsigned int tot = publish_count(sel, s_c, &mask);
  // the workgroup's word goes out before it looks at anybody else's (a << 16 | b of prefix_below: a = selected, b = 0)
  const bool hold = a.test_late != 0 && ((unsigned int)b % 7u) == 3u;  // LII_TEST=emit_late, as k_vhash_emit
  const unsigned long long word = ((unsigned long long)a.epoch << 32) | (tot << 16);
  if (threadIdx.x == 0 && !hold) __hip_atomic_store(a.words + b, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint2 below = prefix_below(a.words, a.epoch, b, s_sum, a.test_late != 0, [&](int q) -> unsigned int {
    const int jq = q * 256 + (int)threadIdx.x;
    unsigned long long mq;
    return publish_count(jq < n && a.selected[jq] != 0, s_r, &mq) << 16;  // (nothing the count reads changes during this launch)
  });
  if (threadIdx.x == 0 && hold) __hip_atomic_store(a.words + b, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned int base = below.x;
  if (b == n_down_blocks - 1 && threadIdx.x == 0) {
    const int ne = (int)(base + tot);
    a.counts_dev[0] = n; a.counts_dev[1] = ne;
    a.counts_host[0] = n; a.counts_host[1] = ne;
  }
  for (int k = 0; k < w; k++) base += s_c[k];
  if (sel) {
    const unsigned int at = base + (unsigned int)__popcll(mask & ((1ull << lane) - 1ull));
    if (!WIRE || a.effect) a.effect[at] = o;
    if (WIRE && a.w_effect) {  // an arbitrary base: the lane's own record, three 16-byte stores
      // (lii_point_noise_set, model 1: the point's own sqrt(R_inv_i) as the fit pass left it, :1051; else the constant of :1050)
      const unsigned int q = a.w_effect_int ? __float_as_uint(a.w_effect_int[j]) : __float_as_uint((float)__builtin_sqrt(1000.0));
      const WireRecord r = wire_record(o.x, o.y, o.z, q, 0u);
      uint4* at_w = a.w_effect + (size_t)at * kWireQuads;
      at_w[0] = r.q[0]; at_w[1] = r.q[1]; at_w[2] = r.q[2];
    }
  }
}

// the save buffer as the rows of a binary PCD (lii_publish_saved_pcd): x y z | normal 0 0 0 | intensity | curvature 0, 32 bytes
__global__ __launch_bounds__(256) void k_pcd_rows(const float4* __restrict__ save, const float* __restrict__ inten, int first, int n, uint4* __restrict__ out) {
  for (int i = (int)(blockIdx.x * 256 + threadIdx.x); i < n; i += (int)(gridDim.x * 256)) {
    const float4 p = save[(size_t)first + i];
    const unsigned int q = inten ? __float_as_uint(inten[(size_t)first + i]) : 0u;
    out[2 * (size_t)i] = make_uint4(__float_as_uint(p.x), __float_as_uint(p.y), __float_as_uint(p.z), 0u);
    out[2 * (size_t)i + 1] = make_uint4(0u, 0u, q, 0u);
  }
}

// ... and map points as the same rows (lii_map_pcd): the intensity is the point's own fourth word
__global__ __launch_bounds__(256) void k_pcd_rows_w(const float4* __restrict__ pts, int first, int n, uint4* __restrict__ out) {
  for (int i = (int)(blockIdx.x * 256 + threadIdx.x); i < n; i += (int)(gridDim.x * 256)) {
    const float4 p = pts[(size_t)first + i];
    out[2 * (size_t)i] = make_uint4(__float_as_uint(p.x), __float_as_uint(p.y), __float_as_uint(p.z), 0u);
    out[2 * (size_t)i + 1] = make_uint4(0u, 0u, __float_as_uint(p.w), 0u);
  }
}

void launch_publish_world(const PublishArgs& a, int down_blocks, const PoseArg& ps, hipStream_t s) {
  const int blocks = a.dense_blocks + down_blocks;
  if (blocks <= 0) return;
  const bool inten = a.dense_int || a.save_int || a.down_int, wire = a.w_dense || a.w_body || a.w_down || a.w_effect;
  const dim3 g((unsigned int)blocks), t(256);
  if (wire && inten) hipLaunchKernelGGL((k_publish_world<true, true>), g, t, 0, s, a, ps);
  else if (wire) hipLaunchKernelGGL((k_publish_world<false, true>), g, t, 0, s, a, ps);
  else if (inten) hipLaunchKernelGGL((k_publish_world<true, false>), g, t, 0, s, a, ps);
  else hipLaunchKernelGGL((k_publish_world<false, false>), g, t, 0, s, a, ps);
}

void launch_pcd_rows(const float4* save, const float* inten, int first, int n, uint4* out, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_pcd_rows, dim3((unsigned int)std::min((n + 255) / 256, 1024)), dim3(256), 0, s, save, inten, first, n, out);
}
void launch_pcd_rows_w(const float4* pts, int first, int n, uint4* out, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_pcd_rows_w, dim3((unsigned int)std::min((n + 255) / 256, 1024)), dim3(256), 0, s, pts, first, n, out);
}

}  // namespace lii
