// libliinit_hip — the registered clouds of a scan (host side): lii_publish_set / _now / _fetch / _saved and the two hooks the
// registration loop calls (publish_enqueue, publish_finish).  Kernel: lii_publish.hip.  Reference: src/laserMapping.cpp:1152-1156
// (publish_frame_world :561-614, publish_frame_body :616-623, publish_effect_world :625-636, pcl_wait_save :594-613).
// lii_publish_wire_* / lii_publish_saved_pcd / lii_pcd_header: the same clouds as the bytes pcl::toROSMsg (:578-586, :619, :632) and
// pcd_writer.writeBinary (:609) produce - a second standing order served by the same launch.
#include "lii_context.h"

using namespace lii_impl;

namespace {
constexpr int kAllClouds = LII_PUB_DENSE | LII_PUB_DOWN | LII_PUB_EFFECT | LII_PUB_BODY;
int cloud_index(int cloud) {
  return cloud == LII_PUB_DENSE ? 0 : cloud == LII_PUB_DOWN ? 1 : cloud == LII_PUB_EFFECT ? 2 : cloud == LII_PUB_BODY ? 3 : -1;
}
// LII_PUB_INTENSITY: the clouds that come with intensities, and their index in Publish::d_int
constexpr int kIntOf[lii_context::Publish::kIntClouds] = {LII_PUB_DENSE, LII_PUB_DOWN, LII_PUB_BODY};
int int_index(int cloud) { return cloud == LII_PUB_DENSE ? 0 : cloud == LII_PUB_DOWN ? 1 : cloud == LII_PUB_BODY ? 2 : -1; }
}  // namespace

// The slots, the counts, the prefix words and the launch's event: what either order needs (created by the first one placed).
static int publish_common(lii_handle h, bool to_host) {
  lii_context::Publish& P = h->pub;
  if (to_host && !h->copy_stream) HIPCHK(h, h->copy_stream.create(hipStreamNonBlocking));
  if (!P.d_counts) {
    HIPCHK(h, P.d_counts.alloc(4));
    HIPCHK(h, hipMemset(P.d_counts, 0, sizeof(int) * 4));
  }
  if (!P.h_counts) {
    HIPCHK(h, P.h_counts.alloc(8, hipHostMallocMapped));
    std::memset(P.h_counts, 0, sizeof(int) * 8);
  }
  if (!P.d_words) {
    HIPCHK(h, P.d_words.alloc(size_t(h->cfg.max_scan_points) / 256 + 2));
    HIPCHK(h, hipMemset(P.d_words, 0, sizeof(unsigned long long) * P.d_words.size()));  // (run number 0 is never used)
  }
  for (int k = 0; k < 2; k++)
    if (!P.ev_pub[k]) HIPCHK(h, P.ev_pub[k].create(hipEventDisableTiming));
  return LII_OK;
}

// An order was placed or changed (both streams drained): the slots start over, the clouds of earlier registrations are forgotten for both orders.
static void publish_restart(lii_context::Publish& P) {
  P.have = -1;
  P.cur = 0;
  P.last_copy[0] = P.last_copy[1] = -1;
  P.wire.last_copy[0] = P.wire.last_copy[1] = -1;
}

int lii_impl::publish_enqueue(lii_handle h, const IekfCtrl* guard, const PoseArg* ps, bool first) {
  lii_context::Publish& P = h->pub;
  lii_context::Publish::Wire& W = P.wire;
  if (!P.any()) return LII_OK;
  hipStream_t s = h->stream;
  const int slot = P.cur;
  const int n_scan = h->n_scan;
  const size_t cap = size_t(h->cfg.max_scan_points);
  if (n_scan < 0 || size_t(n_scan) > cap || h->n_body < 0 || size_t(h->n_body) > cap) return fail(h, LII_ERR_CAPACITY, "publish: the scan exceeds max_scan_points");
  // what each order asks of this launch (an order that is off keeps its settings for a later one: they do not count)
  const int clouds = P.on ? P.clouds : 0, w_clouds = W.on ? W.clouds : 0;
  const int to_host = P.on ? P.to_host : 0, save_capacity = P.on ? P.save_capacity : 0;
  // the slot's clouds of two registrations ago may still be on their way to the host: the launch that overwrites them waits for the copy
  if (P.last_copy[slot] >= 0) HIPCHK(h, hipStreamWaitEvent(s, P.ev_copy[P.last_copy[slot]][slot], 0));
  if (W.last_copy[slot] >= 0) HIPCHK(h, hipStreamWaitEvent(s, W.ev_copy[W.last_copy[slot]][slot], 0));
  if (first && (clouds & LII_PUB_BODY) && n_scan > 0)  // publish_frame_body: the de-skewed scan as it is
    HIPCHK(h, hipMemcpyAsync(P.d_cloud[3][slot], h->d_scan, sizeof(float4) * size_t(n_scan), hipMemcpyDeviceToDevice, s));
  // LII_PUB_INTENSITY: which clouds of this slot get intensities - none when the registered scan has none (the save buffer then gets zeros)
  const bool scan_int = P.on && P.intensity && h->inten.have && n_scan > 0;
  const int int_clouds = !scan_int ? 0 : (clouds & (LII_PUB_DENSE | LII_PUB_BODY)) | ((clouds & LII_PUB_DOWN) && h->inten.body_have ? LII_PUB_DOWN : 0);
  if (first && (int_clouds & LII_PUB_BODY))
    HIPCHK(h, hipMemcpyAsync(P.d_int[2][slot], h->inten.d_scan, sizeof(float) * size_t(n_scan), hipMemcpyDeviceToDevice, s));
  const bool want_dense = (clouds & LII_PUB_DENSE) != 0, want_save = save_capacity > 0;
  const bool want_down = (clouds & LII_PUB_DOWN) != 0, want_effect = (clouds & LII_PUB_EFFECT) != 0;
  PublishArgs a = {};
  a.scan = h->d_scan;
  a.n_scan = n_scan;
  a.dense_blocks = (want_dense || want_save || (w_clouds & (LII_PUB_DENSE | LII_PUB_BODY))) ? (n_scan + 255) / 256 : 0;
  // lii_publish_wire_set: the records of the ordered clouds, with the intensities the scan and its down-sampled cloud carry
  a.w_dense = (w_clouds & LII_PUB_DENSE) ? W.d_cloud[0][slot].get() : nullptr;
  a.w_down = (w_clouds & LII_PUB_DOWN) ? W.d_cloud[1][slot].get() : nullptr;
  a.w_effect = (w_clouds & LII_PUB_EFFECT) ? W.d_cloud[2][slot].get() : nullptr;
  a.w_body = (w_clouds & LII_PUB_BODY) ? W.d_cloud[3][slot].get() : nullptr;
  a.w_scan_int = (w_clouds && h->inten.have && n_scan > 0) ? h->inten.d_scan.get() : nullptr;
  a.w_body_int = (a.w_scan_int && h->inten.body_have) ? h->inten.d_body.get() : nullptr;
  a.w_effect_int = (a.w_effect && h->noise.model == 1) ? h->noise.d_sqrt_rinv() : nullptr;  // (written by the fit passes this launch stands behind)
  a.dense = want_dense ? P.d_cloud[0][slot].get() : nullptr;
  a.save = want_save ? P.d_save.get() : nullptr;
  a.scan_int = scan_int ? h->inten.d_scan.get() : nullptr;
  a.dense_int = (int_clouds & LII_PUB_DENSE) ? P.d_int[0][slot].get() : nullptr;
  a.save_int = want_save ? P.d_save_int.get() : nullptr;  // (once it exists it is appended to by every order: 0.0f where there is nothing to hand on)
  a.body_int = (int_clouds & LII_PUB_DOWN) ? h->inten.d_body.get() : nullptr;
  a.down_int = (int_clouds & LII_PUB_DOWN) ? P.d_int[1][slot].get() : nullptr;
  a.save_cap = P.save_capacity;
  a.save_par = P.save_par;
  a.save_ctl = P.d_save_ctl;
  a.body = h->d_body;
  a.n_body = h->n_body;
  a.n_body_dev = h->n_body_pending ? h->d_nbody.get() : nullptr;
  a.down = want_down ? P.d_cloud[1][slot].get() : nullptr;
  a.selected = h->d_selected;
  a.effect = want_effect ? P.d_cloud[2][slot].get() : nullptr;
  a.words = P.d_words;
  P.epoch = P.epoch == 0xFFFFFFFFu ? 1u : P.epoch + 1u;
  a.epoch = P.epoch;
  a.counts_dev = P.d_counts + 2 * slot;
  a.counts_host = P.h_counts + 4 * slot;
  a.guard = guard;
  a.test_late = h->test_emit_late ? 1 : 0;
  a.seq = h->update_seq;
  const int down_blocks = (want_down || want_effect || (w_clouds & (LII_PUB_DOWN | LII_PUB_EFFECT))) ? std::max(1, (h->n_body + 255) / 256) : 0;
  if (size_t(down_blocks) > P.d_words.size()) return fail(h, LII_ERR_CAPACITY, "publish: more workgroups than prefix words");
  P.kp_idx = -1;
  if (a.dense_blocks + down_blocks > 0) {
    if (h->prof.kp_active) { P.kp_idx = h->prof.kp_n; const int r = kp_mark(h, LII_KP_PUBLISH); if (r != LII_OK) return r; }
    launch_publish_world(a, down_blocks, ps ? *ps : PoseArg{}, s);
    HIPCHK(h, hipGetLastError());
    if (want_save && a.dense_blocks > 0) P.save_par ^= 1;  // (the launch has moved the offset to the other word, whether it appended or not)
    if (h->prof.kp_active) { const int r = kp_mark(h, LII_KP_KINDS); if (r != LII_OK) return r; }
  }
  HIPCHK(h, hipEventRecord(P.ev_pub[slot], s));
  const int n_of[lii_context::Publish::kClouds] = {n_scan, h->n_body, h->n_body, n_scan};  // (down-sampled / effect: the bound; the counts travel in h_counts)
  if (to_host || (W.on && W.to_host)) HIPCHK(h, hipStreamWaitEvent(h->copy_stream, P.ev_pub[slot], 0));
  if (to_host) {
    if (int_clouds) {  // (in front of the clouds' copies: the event recorded last for the slot lies behind them as well)
      const int n_int[lii_context::Publish::kIntClouds] = {n_scan, h->n_body, n_scan};
      for (int k = 0; k < lii_context::Publish::kIntClouds; k++)
        if ((int_clouds & kIntOf[k]) && n_int[k] > 0)
          HIPCHK(h, hipMemcpyAsync(P.h_int[k][slot], P.d_int[k][slot], sizeof(float) * size_t(n_int[k]), hipMemcpyDeviceToHost, h->copy_stream));
      HIPCHK(h, hipEventRecord(P.ev_int[slot], h->copy_stream));
    }
    for (int c = 0; c < lii_context::Publish::kClouds; c++) {
      if (!(clouds & (1 << c))) continue;
      if (n_of[c] > 0)
        HIPCHK(h, hipMemcpyAsync(P.h_cloud[c][slot], P.d_cloud[c][slot], sizeof(float4) * size_t(n_of[c]), hipMemcpyDeviceToHost, h->copy_stream));
      HIPCHK(h, hipEventRecord(P.ev_copy[c][slot], h->copy_stream));
      P.last_copy[slot] = c;
    }
  }
  if (W.on && W.to_host) {  // the records, behind the float4 clouds on the same stream, each behind an event of its own
    for (int c = 0; c < lii_context::Publish::kClouds; c++) {
      if (!(w_clouds & (1 << c))) continue;
      if (n_of[c] > 0)
        HIPCHK(h, hipMemcpyAsync(W.h_cloud[c][slot], W.d_cloud[c][slot], sizeof(uint4) * kWireQuads * size_t(n_of[c]), hipMemcpyDeviceToHost, h->copy_stream));
      HIPCHK(h, hipEventRecord(W.ev_copy[c][slot], h->copy_stream));
      W.last_copy[slot] = c;
    }
  }
  h->scan_buf_idle = false;  // (the launch and the body copy read the current scan buffer: lii_scan_upload_next orders its transfer behind them)
  P.n_scan_at[slot] = n_scan;
  P.clouds_at[slot] = clouds;
  P.int_at[slot] = int_clouds;
  W.clouds_at[slot] = w_clouds;
  return LII_OK;
}

void lii_impl::publish_finish(lii_handle h) {
  lii_context::Publish& P = h->pub;
  if (!P.any()) return;
  P.have = P.cur;
  P.cur ^= 1;
}

extern "C" {

int lii_publish_set(lii_handle h, const lii_publish_opts* opts) {
  if (!h) return LII_ERR_INVALID;
  if (opts && (opts->struct_size != sizeof(lii_publish_opts) || (opts->clouds & ~(kAllClouds | LII_PUB_INTENSITY)) ||
               ((opts->clouds & LII_PUB_INTENSITY) && !(opts->clouds & (LII_PUB_DENSE | LII_PUB_DOWN | LII_PUB_BODY))) || (opts->to_host != 0 && opts->to_host != 1) || opts->save_capacity < 0))
    return fail(h, LII_ERR_INVALID, "lii_publish_set: bad lii_publish_opts (struct_size, unknown cloud bits, LII_PUB_INTENSITY without DENSE / DOWN / BODY, to_host, save_capacity)");
  if (h->in_wait_hook) return fail(h, LII_ERR_STATE, "lii_publish_set: a registration is under way (lii_scan_job::while_waiting)");
  lii_internal_prearm_cancel(h);  // (a pre-armed de-skew launch waiting on the stream is told to end: this entry point uses the stream)
  lii_context::Publish& P = h->pub;
  if (!opts || (opts->clouds == 0 && opts->save_capacity == 0)) {  // off: the buffers stay for a later order
    P.on = false;
    P.have = -1;
    return LII_OK;
  }
  if (h->net.comm || h->net.n_ranks > 1) return fail(h, LII_ERR_STATE, "lii_publish_set: single rank only for now (a communicator is attached)");
  if (h->host_solve) return fail(h, LII_ERR_STATE, "lii_publish_set: single rank only for now - not with LII_TEST=host_solve (the host-driven loop has no control block to publish from)");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));  // (a launch of the previous order may still read what is replaced below)
  if (h->copy_stream) HIPCHK(h, hipStreamSynchronize(h->copy_stream));
  P.on = false;
  P.have = -1;
  const size_t cap = size_t(h->cfg.max_scan_points);
  for (int c = 0; c < lii_context::Publish::kClouds; c++) {
    if (!(opts->clouds & (1 << c))) continue;
    for (int k = 0; k < 2; k++) {
      if (!P.d_cloud[c][k]) HIPCHK(h, P.d_cloud[c][k].alloc(cap));
      if (opts->to_host && !P.h_cloud[c][k]) HIPCHK(h, P.h_cloud[c][k].alloc(cap, hipHostMallocDefault));
      if (opts->to_host && !P.ev_copy[c][k]) HIPCHK(h, P.ev_copy[c][k].create(hipEventDisableTiming));
    }
  }
  const bool want_int = (opts->clouds & LII_PUB_INTENSITY) != 0;
  for (int c = 0; want_int && c < lii_context::Publish::kIntClouds; c++) {
    if (!(opts->clouds & kIntOf[c])) continue;
    for (int k = 0; k < 2; k++) {
      if (!P.d_int[c][k]) HIPCHK(h, P.d_int[c][k].alloc(cap));
      if (opts->to_host && !P.h_int[c][k]) HIPCHK(h, P.h_int[c][k].alloc(cap, hipHostMallocDefault));
    }
  }
  for (int k = 0; want_int && opts->to_host && k < 2; k++)
    if (!P.ev_int[k]) HIPCHK(h, P.ev_int[k].create(hipEventDisableTiming));
  { const int rc = publish_common(h, opts->to_host != 0); if (rc != LII_OK) return rc; }
  if (opts->save_capacity > 0 && P.d_save.size() != size_t(opts->save_capacity)) {  // the first order that asks for it (another capacity: a new, empty buffer)
    HIPCHK(h, P.d_save.grow(size_t(opts->save_capacity)));
    if (!P.d_save_ctl) HIPCHK(h, P.d_save_ctl.alloc(4));
    HIPCHK(h, hipMemset(P.d_save_ctl, 0, sizeof(int) * 4));
    P.save_par = 0;
    P.d_save_int.reset();  // (a new, empty save buffer: its intensities follow below)
  }
  if (want_int && opts->save_capacity > 0 && !P.d_save_int) {
    // the intensities of the save buffer, point for point; what an order without the bit has appended so far has 0.0f
    HIPCHK(h, P.d_save_int.alloc(size_t(opts->save_capacity)));
    HIPCHK(h, hipMemset(P.d_save_int, 0, sizeof(float) * size_t(opts->save_capacity)));
  }
  P.intensity = want_int;
  P.clouds = opts->clouds & kAllClouds;
  P.to_host = opts->to_host;
  P.save_capacity = opts->save_capacity;
  publish_restart(P);  // (both streams were drained above)
  P.on = true;
  return LII_OK;
}

int lii_publish_wire_set(lii_handle h, const lii_wire_opts* opts) {
  if (!h) return LII_ERR_INVALID;
  if (opts && (opts->struct_size != sizeof(lii_wire_opts) || (opts->clouds & ~kAllClouds) || (opts->to_host != 0 && opts->to_host != 1) || opts->reserved != 0))
    return fail(h, LII_ERR_INVALID, "lii_publish_wire_set: bad lii_wire_opts (struct_size, unknown cloud bits - LII_PUB_INTENSITY is one here -, to_host, reserved)");
  if (h->in_wait_hook) return fail(h, LII_ERR_STATE, "lii_publish_wire_set: a registration is under way (lii_scan_job::while_waiting)");
  lii_internal_prearm_cancel(h);  // (a pre-armed de-skew launch waiting on the stream is told to end: this entry point uses the stream)
  lii_context::Publish& P = h->pub;
  lii_context::Publish::Wire& W = P.wire;
  if (!opts || opts->clouds == 0) {  // off: the buffers stay for a later order
    W.on = false;
    P.have = -1;
    return LII_OK;
  }
  if (h->net.comm || h->net.n_ranks > 1) return fail(h, LII_ERR_STATE, "lii_publish_wire_set: single rank only for now (a communicator is attached)");
  if (h->host_solve) return fail(h, LII_ERR_STATE, "lii_publish_wire_set: single rank only for now - not with LII_TEST=host_solve (the host-driven loop has no control block to publish from)");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));  // (a launch of the previous order may still write what is replaced below)
  if (h->copy_stream) HIPCHK(h, hipStreamSynchronize(h->copy_stream));
  W.on = false;
  P.have = -1;
  const size_t quads = size_t(kWireQuads) * size_t(h->cfg.max_scan_points);
  for (int c = 0; c < lii_context::Publish::kClouds; c++) {
    if (!(opts->clouds & (1 << c))) continue;
    for (int k = 0; k < 2; k++) {
      if (!W.d_cloud[c][k]) HIPCHK(h, W.d_cloud[c][k].alloc(quads));
      if (opts->to_host && !W.h_cloud[c][k]) HIPCHK(h, W.h_cloud[c][k].alloc(quads, hipHostMallocDefault));
      if (opts->to_host && !W.ev_copy[c][k]) HIPCHK(h, W.ev_copy[c][k].create(hipEventDisableTiming));
    }
  }
  { const int rc = publish_common(h, opts->to_host != 0); if (rc != LII_OK) return rc; }
  W.clouds = opts->clouds;
  W.to_host = opts->to_host;
  publish_restart(P);  // (both streams were drained above)
  W.on = true;
  return LII_OK;
}

int lii_publish_wire_fetch(lii_handle h, int32_t cloud, const void** host_bytes, const void** dev_bytes, int32_t* n_points) {
  if (!h || !n_points) return fail(h, LII_ERR_INVALID, "lii_publish_wire_fetch: bad arguments");
  const int c = cloud_index(cloud);
  if (c < 0) return fail(h, LII_ERR_INVALID, "lii_publish_wire_fetch: unknown cloud");
  lii_context::Publish& P = h->pub;
  lii_context::Publish::Wire& W = P.wire;
  if (!W.on || P.have < 0) return fail(h, LII_ERR_STATE, "lii_publish_wire_fetch: no registration since the order (lii_publish_wire_set)");
  const int slot = P.have;
  if (!(W.clouds_at[slot] & cloud)) return fail(h, LII_ERR_STATE, "lii_publish_wire_fetch: this cloud was not ordered");
  // this cloud's event only, as lii_publish_fetch: it may be called from lii_scan_job::while_waiting of the next call
  HIPCHK(h, hipEventSynchronize(W.to_host ? W.ev_copy[c][slot] : P.ev_pub[slot]));
  std::atomic_thread_fence(std::memory_order_acquire);
  const volatile int* hc = P.h_counts + 4 * slot;
  *n_points = (c == 0 || c == 3) ? P.n_scan_at[slot] : hc[c == 1 ? 0 : 1];
  if (host_bytes) *host_bytes = W.to_host ? W.h_cloud[c][slot].get() : nullptr;
  if (dev_bytes) *dev_bytes = W.d_cloud[c][slot].get();
  return LII_OK;
}

int lii_publish_wire_layout(lii_wire_layout* out) {
  if (!out || out->struct_size != sizeof(lii_wire_layout)) return LII_ERR_INVALID;
  static const char* const names[LII_WIRE_FIELDS] = {"x", "y", "z", "normal_x", "normal_y", "normal_z", "intensity", "curvature"};
  static const int offsets[LII_WIRE_FIELDS] = {0, 4, 8, 16, 20, 24, 32, 36};
  std::memset(out, 0, sizeof(*out));
  out->struct_size = sizeof(lii_wire_layout);
  out->point_step = LII_WIRE_POINT_STEP;
  out->n_fields = LII_WIRE_FIELDS;
  out->pcd_row_bytes = LII_WIRE_PCD_ROW;
  for (int k = 0; k < LII_WIRE_FIELDS; k++) {
    std::strncpy(out->fields[k].name, names[k], sizeof(out->fields[k].name) - 1);
    out->fields[k].offset = offsets[k];
    out->fields[k].datatype = LII_WIRE_FLOAT32;
    out->fields[k].count = 1;
    out->fields[k].pcd_offset = 4 * k;  // (PCDWriter::writeBinary packs the fields without padding)
  }
  return LII_OK;
}

int lii_pcd_header(int32_t n_points, char* out, int32_t capacity, int32_t* len) {
  if (n_points < 0 || !len || (out && capacity < 0)) return LII_ERR_INVALID;
  char text[512];
  const int n = std::snprintf(text, sizeof(text),
                              "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z normal_x normal_y normal_z intensity curvature\n"
                              "SIZE 4 4 4 4 4 4 4 4\nTYPE F F F F F F F F\nCOUNT 1 1 1 1 1 1 1 1\nWIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA binary\n",
                              n_points, n_points);
  if (n <= 0 || size_t(n) >= sizeof(text)) return LII_ERR_INVALID;
  *len = n;
  if (!out) return LII_OK;
  if (capacity < n) return LII_ERR_CAPACITY;
  std::memcpy(out, text, size_t(n));
  if (capacity > n) out[n] = 0;
  return LII_OK;
}

int lii_publish_saved_pcd(lii_handle h, void* rows_out, int64_t capacity_bytes, int32_t* n_points, int32_t clear) {
  if (!h || !n_points) return fail(h, LII_ERR_INVALID, "lii_publish_saved_pcd: bad arguments");
  if (h->in_wait_hook) return fail(h, LII_ERR_STATE, "lii_publish_saved_pcd: a registration is under way (lii_scan_job::while_waiting)");
  lii_internal_prearm_cancel(h);  // (a pre-armed de-skew launch waiting on the stream is told to end: this entry point uses the stream)
  lii_context::Publish& P = h->pub;
  if (!P.d_save) return fail(h, LII_ERR_STATE, "lii_publish_saved_pcd: no save buffer (lii_publish_opts::save_capacity)");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  int ctl[4] = {0, 0, 0, 0};
  HIPCHK(h, hipMemcpy(ctl, P.d_save_ctl, sizeof(ctl), hipMemcpyDeviceToHost));
  const int cnt = ctl[P.save_par];
  *n_points = cnt;
  if (cnt < 0 || size_t(cnt) > P.d_save.size()) return fail(h, LII_ERR_HIP, "lii_publish_saved_pcd: append offset out of range");
  if (rows_out) {
    if (capacity_bytes < int64_t(LII_WIRE_PCD_ROW) * cnt) return fail(h, LII_ERR_CAPACITY, "lii_publish_saved_pcd: capacity too small");
    if (cnt > 0 && !P.wire.d_pcd) HIPCHK(h, P.wire.d_pcd.alloc(2 * size_t(kPcdChunkRows)));
    // repacked on the device, chunk by chunk through the staging area (the copy of a chunk ends before the next launch overwrites it)
    for (int first = 0; first < cnt; first += kPcdChunkRows) {
      const int n = std::min(kPcdChunkRows, cnt - first);
      launch_pcd_rows(P.d_save, P.d_save_int ? P.d_save_int.get() : nullptr, first, n, P.wire.d_pcd, h->stream);
      HIPCHK(h, hipGetLastError());
      HIPCHK(h, hipMemcpyAsync(static_cast<char*>(rows_out) + size_t(LII_WIRE_PCD_ROW) * size_t(first), P.wire.d_pcd, size_t(LII_WIRE_PCD_ROW) * size_t(n), hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
    }
  }
  if (clear) {
    HIPCHK(h, hipMemset(P.d_save_ctl, 0, sizeof(int) * 4));
    P.save_par = 0;
  }
  if (ctl[2]) return fail(h, LII_ERR_CAPACITY, "lii_publish_saved_pcd: the save buffer overflowed - at least one scan was not appended (what it held is intact)");
  return LII_OK;
}

int lii_publish_now(lii_handle h, const lii_state* state) {
  if (!h || !state) return fail(h, LII_ERR_INVALID, "lii_publish_now: bad arguments");
  if (h->in_wait_hook) return fail(h, LII_ERR_STATE, "lii_publish_now: a registration is under way (lii_scan_job::while_waiting)");
  lii_internal_prearm_cancel(h);  // (a pre-armed de-skew launch waiting on the stream is told to end: this entry point uses the stream)
  lii_context::Publish& P = h->pub;
  if (!P.any()) return fail(h, LII_ERR_STATE, "lii_publish_now: nothing is ordered (lii_publish_set, lii_publish_wire_set)");
  { const int rcm = scan_materialize(h); if (rcm != LII_OK) return rcm; }
  if ((((P.on ? P.clouds : 0) | (P.wire.on ? P.wire.clouds : 0)) & (LII_PUB_DOWN | LII_PUB_EFFECT)) && h->n_body <= 0)
    return fail(h, LII_ERR_STATE, "lii_publish_now: no down-sampled scan (call lii_downsample / lii_downsample_skip)");
  const PoseArg ps = pose_of(*state);
  const int rc = publish_enqueue(h, nullptr, &ps, true);
  if (rc != LII_OK) return rc;
  publish_finish(h);
  return LII_OK;
}

int lii_publish_fetch(lii_handle h, int32_t cloud, const float** host_float4, const void** dev_float4, int32_t* n) {
  if (!h || !n) return fail(h, LII_ERR_INVALID, "lii_publish_fetch: bad arguments");
  const int c = cloud_index(cloud);
  if (c < 0) return fail(h, LII_ERR_INVALID, "lii_publish_fetch: unknown cloud");
  lii_context::Publish& P = h->pub;
  if (!P.on || P.have < 0) return fail(h, LII_ERR_STATE, "lii_publish_fetch: no registration since the order (lii_publish_set)");
  const int slot = P.have;
  if (!(P.clouds_at[slot] & cloud)) return fail(h, LII_ERR_STATE, "lii_publish_fetch: this cloud was not ordered");
  // this cloud's event only: neither the handle's stream nor a pre-armed launch behind it is touched
  HIPCHK(h, hipEventSynchronize(P.to_host ? P.ev_copy[c][slot] : P.ev_pub[slot]));
  std::atomic_thread_fence(std::memory_order_acquire);
  const volatile int* hc = P.h_counts + 4 * slot;
  *n = (c == 0 || c == 3) ? P.n_scan_at[slot] : hc[c == 1 ? 0 : 1];
  if (host_float4) *host_float4 = P.to_host ? reinterpret_cast<const float*>(P.h_cloud[c][slot].get()) : nullptr;
  if (dev_float4) *dev_float4 = P.d_cloud[c][slot].get();
  return LII_OK;
}

int lii_publish_fetch_intensity(lii_handle h, int32_t cloud, const float** host_float, const void** dev_float, int32_t* n) {
  if (!h || !n) return fail(h, LII_ERR_INVALID, "lii_publish_fetch_intensity: bad arguments");
  const int c = cloud_index(cloud), k = int_index(cloud);
  // (the effect cloud is not served: the reference overwrites its intensity with sqrt(R_inv), src/laserMapping.cpp:1051 - nothing of the sensor's is left)
  if (c < 0 || k < 0) return fail(h, LII_ERR_INVALID, "lii_publish_fetch_intensity: LII_PUB_DENSE, LII_PUB_DOWN or LII_PUB_BODY");
  lii_context::Publish& P = h->pub;
  if (!P.on || P.have < 0) return fail(h, LII_ERR_STATE, "lii_publish_fetch_intensity: no registration since the order (lii_publish_set)");
  const int slot = P.have;
  if (!P.intensity || !(P.clouds_at[slot] & cloud)) return fail(h, LII_ERR_STATE, "lii_publish_fetch_intensity: this cloud was not ordered with LII_PUB_INTENSITY");
  if (!(P.int_at[slot] & cloud)) return fail(h, LII_ERR_STATE, "lii_publish_fetch_intensity: the registered scan had no intensities attached");
  // the intensities' event only, as lii_publish_fetch: it may be called from lii_scan_job::while_waiting of the next call
  HIPCHK(h, hipEventSynchronize(P.to_host ? P.ev_int[slot] : P.ev_pub[slot]));
  std::atomic_thread_fence(std::memory_order_acquire);
  const volatile int* hc = P.h_counts + 4 * slot;
  *n = k == 1 ? hc[0] : P.n_scan_at[slot];
  if (host_float) *host_float = P.to_host ? P.h_int[k][slot].get() : nullptr;
  if (dev_float) *dev_float = P.d_int[k][slot].get();
  return LII_OK;
}

int lii_publish_saved_intensity(lii_handle h, float* out, int32_t capacity, int32_t* n) {
  if (!h || !n) return fail(h, LII_ERR_INVALID, "lii_publish_saved_intensity: bad arguments");
  if (h->in_wait_hook) return fail(h, LII_ERR_STATE, "lii_publish_saved_intensity: a registration is under way (lii_scan_job::while_waiting)");
  lii_internal_prearm_cancel(h);  // (a pre-armed de-skew launch waiting on the stream is told to end: this entry point uses the stream)
  lii_context::Publish& P = h->pub;
  if (!P.d_save || !P.d_save_int) return fail(h, LII_ERR_STATE, "lii_publish_saved_intensity: no save buffer with intensities (lii_publish_opts::save_capacity with LII_PUB_INTENSITY)");
  HIPCHK(h, hipStreamSynchronize(h->stream));
  int ctl[4] = {0, 0, 0, 0};
  HIPCHK(h, hipMemcpy(ctl, P.d_save_ctl, sizeof(ctl), hipMemcpyDeviceToHost));
  const int cnt = ctl[P.save_par];
  *n = cnt;
  if (cnt < 0 || size_t(cnt) > P.d_save_int.size()) return fail(h, LII_ERR_HIP, "lii_publish_saved_intensity: append offset out of range");
  if (out) {
    if (capacity < cnt) return fail(h, LII_ERR_CAPACITY, "lii_publish_saved_intensity: capacity too small");
    if (cnt > 0) HIPCHK(h, hipMemcpy(out, P.d_save_int, sizeof(float) * size_t(cnt), hipMemcpyDeviceToHost));
  }
  if (ctl[2]) return fail(h, LII_ERR_CAPACITY, "lii_publish_saved_intensity: the save buffer overflowed - at least one scan was not appended (what it held is intact)");
  return LII_OK;
}

int lii_publish_saved(lii_handle h, float* out_float4, int32_t capacity, int32_t* n, int32_t clear) {
  if (!h || !n) return fail(h, LII_ERR_INVALID, "lii_publish_saved: bad arguments");
  if (h->in_wait_hook) return fail(h, LII_ERR_STATE, "lii_publish_saved: a registration is under way (lii_scan_job::while_waiting)");
  lii_internal_prearm_cancel(h);  // (a pre-armed de-skew launch waiting on the stream is told to end: this entry point uses the stream)
  lii_context::Publish& P = h->pub;
  if (!P.d_save) return fail(h, LII_ERR_STATE, "lii_publish_saved: no save buffer (lii_publish_opts::save_capacity)");
  HIPCHK(h, hipStreamSynchronize(h->stream));
  int ctl[4] = {0, 0, 0, 0};
  HIPCHK(h, hipMemcpy(ctl, P.d_save_ctl, sizeof(ctl), hipMemcpyDeviceToHost));
  const int cnt = ctl[P.save_par];
  *n = cnt;
  if (cnt < 0 || size_t(cnt) > P.d_save.size()) return fail(h, LII_ERR_HIP, "lii_publish_saved: append offset out of range");
  if (out_float4) {
    if (capacity < cnt) return fail(h, LII_ERR_CAPACITY, "lii_publish_saved: capacity too small");
    if (cnt > 0) HIPCHK(h, hipMemcpy(out_float4, P.d_save, sizeof(float4) * size_t(cnt), hipMemcpyDeviceToHost));
  }
  if (clear) {
    HIPCHK(h, hipMemset(P.d_save_ctl, 0, sizeof(int) * 4));
    P.save_par = 0;
  }
  if (ctl[2]) return fail(h, LII_ERR_CAPACITY, "lii_publish_saved: the save buffer overflowed - at least one scan was not appended (what it held is intact)");
  return LII_OK;
}

}  // extern "C"
