// Feature extraction behind the whole-message ingest (lii_feature.hip) and what it shares with lii_ingest.hip: the frame table a message's
// last launch writes into mapped host memory.  Internal; not the C-ABI.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "lii_owned.h"

namespace lii {

constexpr int kMaxLines = 128;   // MAX_LINE_NUM, src/preprocess.cpp:114
constexpr int kMaxFrames = 64;

struct IngestTable {  // written by k_cut_plan / k_whole_apply / k_feat_emit into mapped host memory
  int n_frames;
  int n_kept;        // pl_surf.size()
  int n_emitted;     // points inside frames
  int unsorted;      // 1: the kept points did NOT arrive in ascending time order (k_cut_apply)
  int first[kMaxFrames];   // sorted index of the first point of frame c
  int last[kMaxFrames];    // sorted index of the boundary point of frame c
  double begin_ms[kMaxFrames];
  double delta[kMaxFrames];  // stamp_ms - last_frame_end_time while frame c is filled
  double tail_ms[kMaxFrames];  // adjusted curvature of the frame's last (boundary) point
  int n_corn;        // pl_corn.size() (a message ingested under lii_ingest_set_features; 0 otherwise)
  int n_feat_lines;  // lines give_feature ran on
};

// The constants of Preprocess::Preprocess (src/preprocess.cpp:10-34).  disB is never initialised there (disA is set twice): 0 here.
// The four cosines are formed once on the host (lii_ingest_set_features).
struct FeatureParams {
  int lidar_type, n_scans, pfn;
  double blind;
  double jump_up_limit, jump_down_limit, cos160, smallp_intersect;
};
FeatureParams feature_params_default();

// Device memory of one message context, created by the first message that is ingested under the order (sized like the context's
// per-point buffers: every array holds one element per raw point).
struct FeatureBufs {
  DevBuf<float4> d_lp;            // the kept points, partitioned by line (message order kept within a line)
  DevBuf<unsigned int> d_lidx;    // ... and the raw index of each
  DevBuf<double> d_range, d_dista, d_inter;  // orgtype::range / dista / intersect
  DevBuf<uint8_t> d_ftype, d_fire;           // orgtype::ftype; pass 3's firings
  DevBuf<float4> d_surf_stage, d_corn_stage;  // per line, at the line's offset: what the line emits
  DevBuf<unsigned int> d_corn_sidx;           // raw index of each staged corner
  DevBuf<float4> d_corn;          // pl_corn (x, y, z, curvature), line-major
  DevBuf<float> d_corn_int;       // ... and its intensities
  DevBuf<int> d_line;             // 4 x kMaxLines: points, surface points, corners per line; 1 where the passes ran
  DevBuf<int> d_hist;             // kMaxLines per chunk of 256 kept points: the partition's counts, then their prefix over the chunks
  size_t cap() const { return d_lp.size(); }
};
hipError_t feature_reserve(FeatureBufs* fb, size_t cap);

// Enqueued on `s` behind the decode, the scan of the keep flags (rank) and the compaction (kept_idx: raw indices of the kept points in
// message order): partition by line, the four passes of give_feature per line, compaction of pl_surf into `frames` and of pl_corn
// into fb.d_corn, the frame table.  line_of_raw: ring / line per RAW point.  int_kind / int_off / int_step: how a raw record yields the
// corners' intensity (0: a float, 1: a uint8, 2: none).
void feature_launch(const FeatureBufs& fb, const FeatureParams& p, const float4* pts, const uint8_t* line_of_raw, const unsigned int* kept_idx,
                    const unsigned int* rank, int n, const uint8_t* raw, int int_step, int int_off, int int_kind, double stamp_ms,
                    float4* frames, IngestTable* dev_tab, IngestTable* host_tab, hipStream_t s);

}  // namespace lii
