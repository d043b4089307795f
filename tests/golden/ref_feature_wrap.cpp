// TEST INFRASTRUCTURE ONLY (our own text).  extern "C" wrapper around the UNMODIFIED reference Preprocess class with feature extraction
// enabled: compiled by tests/golden/make_feature_fixture.py together with the reference's src/preprocess.cpp, where it lies, against
// oracle/ref_shim_pre into oracle/_ref/libref_feature.so.  Two reads of the reference decide results and touch memory nobody wrote:
// Preprocess::disB (the constructor sets disA twice) and types[plsize - 1].dista (plane_judge pushes it whenever a group runs to the end
// of a line).  The wrapper pins both: the object is constructed by placement-new in calloc'd storage (disB = 0), and every typess[j] is
// preset to n + 1 elements with dista = `dista_preset` before process() - types.clear(); types.resize() then reuses that storage, and
// orgtype's constructor leaves dista alone.
#include "preprocess.h"

namespace {
Preprocess* make(int lidar_type, int n_scans, int pfn, double blind, int n, double dista_preset) {
  void* mem = std::calloc(1, sizeof(Preprocess));
  Preprocess* pre = new (mem) Preprocess();
  pre->set(true, lidar_type, blind, pfn);
  pre->N_SCANS = n_scans;
  for (int j = 0; j < 128; j++) {
    pre->typess[j].resize((size_t)n + 1);
    for (auto& t : pre->typess[j]) t.dista = dista_preset;
  }
  return pre;
}
void drop(Preprocess* pre) {
  pre->~Preprocess();
  std::free(pre);
}
int emit(Preprocess* pre, float* surf4, float* corn5, int cap, int* n_corn) {
  const int ns = (int)pre->pl_surf.size(), nc = (int)pre->pl_corn.size();
  if (ns > cap || nc > cap) return -2;
  for (int i = 0; i < ns; i++) {
    const PointType& p = pre->pl_surf.points[i];
    surf4[4 * i + 0] = p.x; surf4[4 * i + 1] = p.y; surf4[4 * i + 2] = p.z; surf4[4 * i + 3] = p.curvature;
    if (p.intensity != 0.f) return -3;  // (the emitted surface points carry no intensity)
  }
  for (int i = 0; i < nc; i++) {
    const PointType& p = pre->pl_corn.points[i];
    corn5[5 * i + 0] = p.x; corn5[5 * i + 1] = p.y; corn5[5 * i + 2] = p.z; corn5[5 * i + 3] = p.intensity; corn5[5 * i + 4] = p.curvature;
  }
  *n_corn = nc;
  return ns;
}
}  // namespace

extern "C" {

// fields7: point_step, x, y, z, intensity, time, ring.  Returns pl_surf.size() (< 0: error), *n_corn = pl_corn.size().
int ref_features_pcl2(const unsigned char* data, int n, const int* fields7, int lidar_type, int n_scans, int pfn, double blind,
                      double dista_preset, float* surf4, float* corn5, int cap, int* n_corn) {
  if (lidar_type != VELO && lidar_type != OUSTER) return -1;
  auto msg = std::make_shared<sensor_msgs::PointCloud2>();
  msg->point_step = fields7[0];
  msg->width = n;
  msg->row_step = n * fields7[0];
  msg->data.assign(data, data + (size_t)n * fields7[0]);
  const char* names[6] = {"x", "y", "z", "intensity", lidar_type == VELO ? "time" : "t", "ring"};
  for (int k = 0; k < 6; k++) {
    sensor_msgs::PointField f;
    f.name = names[k];
    f.offset = fields7[1 + k];
    msg->fields.push_back(f);
  }
  Preprocess* pre = make(lidar_type, n_scans, pfn, blind, n, dista_preset);
  PointCloudXYZI::Ptr ptr(new PointCloudXYZI());
  pre->process(msg, ptr);
  const int rc = ptr->size() == pre->pl_surf.size() ? emit(pre, surf4, corn5, cap, n_corn) : -4;
  drop(pre);
  return rc;
}

// fields8: point_step, offset_time, x, y, z, reflectivity, tag, line
int ref_features_livox(const unsigned char* data, int n, const int* fields8, int n_scans, int pfn, double blind, double dista_preset,
                       float* surf4, float* corn5, int cap, int* n_corn) {
  auto msg = std::make_shared<livox_ros_driver::CustomMsg>();
  msg->point_num = n;
  msg->points.resize(n);
  for (int i = 0; i < n; i++) {
    const unsigned char* p = data + (size_t)i * fields8[0];
    livox_ros_driver::CustomPoint& q = msg->points[i];
    std::memcpy(&q.offset_time, p + fields8[1], 4);
    std::memcpy(&q.x, p + fields8[2], 4);
    std::memcpy(&q.y, p + fields8[3], 4);
    std::memcpy(&q.z, p + fields8[4], 4);
    q.reflectivity = p[fields8[5]];
    q.tag = p[fields8[6]];
    q.line = p[fields8[7]];
  }
  Preprocess* pre = make(AVIA, n_scans, pfn, blind, n, dista_preset);
  PointCloudXYZI::Ptr ptr(new PointCloudXYZI());
  pre->process(msg, ptr);
  const int rc = ptr->size() == pre->pl_surf.size() ? emit(pre, surf4, corn5, cap, n_corn) : -4;
  drop(pre);
  return rc;
}

}  // extern "C"
