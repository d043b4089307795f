// The residual gate and the Jacobian row of one point, as the units that form rows share it: the fit launch of the registration pass
// (lii_fit.hip) and the batched pose refinement (lii_refine.hip).  Device code only; double precision, contraction off (see Makefile).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "lii_device.h"

namespace lii {

// residual gate + Jacobian row of one point (src/laserMapping.cpp:999-1010, :1035-1071)
struct RowOut {
  double h[12];
  double z;
  bool sel;
};
// NOISE (lii_point_noise_set, model 1): a selected point also yields R_inv_i = 1 / sigma^2_i (`w`), the weight src/laserMapping.cpp:1039-1042
// computes and :1050 discards.  calcBodyVar (:158-181) gives the point var = range_var d d^T + A diag(s^2) A^T in the IMU frame, d the ray,
// A = [p_I]x N with N a basis of the ray's tangent plane - (1, 1, -(dx + dy) / dz): NaN for any point with z = 0 - and the update needs
// n^T (R_end var R_end^T) n alone.  N is orthonormal, so A diag(s^2) A^T = s^2 r^2 (I - d d^T) whatever the basis, and with t = R_end^T n:
//   sigma^2_i = LASER_POINT_COV + range_var (t . p_I)^2 / r^2 + s^2 |p_I x t|^2      (the radial term 0 when r^2 == 0)
// finite everywhere, from values the row holds already: p_I x t is h[0 .. 2].
template <bool NOISE>
__device__ __forceinline__ void residual_row(const PoseArg& ps, int imu_en, double bx, double by, double bz, double ix,
                                             double iy, double iz, float wx, float wy, float wz, double pa, double pbn,
                                             double pc, double pd, RowOut& o, const NoiseArg& na, double& w) {
  float pd2 = (float)(pa * wx + pbn * wy + pc * wz + pd);
  double pbnorm = sqrt(bx * bx + by * by + bz * bz);
  float s = (float)(1 - 0.9 * fabsf(pd2) / sqrt(pbnorm));
  if (s > 0.9) {
    o.sel = true;
    // normvec stores n̂ as float (:1004-1006); the Jacobian reads those floats back (:1046-1047)
    double nx = (double)(float)pa, ny = (double)(float)pbn, nz = (double)(float)pc;
    double tx = ps.R[0] * nx + ps.R[3] * ny + ps.R[6] * nz;  // R_end^T n̂
    double ty = ps.R[1] * nx + ps.R[4] * ny + ps.R[7] * nz;
    double tz = ps.R[2] * nx + ps.R[5] * ny + ps.R[8] * nz;
    o.h[0] = -iz * ty + iy * tz;  // [p_I]x R_end^T n̂
    o.h[1] = iz * tx - ix * tz;
    o.h[2] = -iy * tx + ix * ty;
    o.h[3] = nx; o.h[4] = ny; o.h[5] = nz;
    if (imu_en) {
      double ux = ps.RLI[0] * tx + ps.RLI[3] * ty + ps.RLI[6] * tz;  // R_LI^T R_end^T n̂
      double uy = ps.RLI[1] * tx + ps.RLI[4] * ty + ps.RLI[7] * tz;
      double uz = ps.RLI[2] * tx + ps.RLI[5] * ty + ps.RLI[8] * tz;
      o.h[6] = -bz * uy + by * uz;  // [p_L]x ...
      o.h[7] = bz * ux - bx * uz;
      o.h[8] = -by * ux + bx * uy;
      o.h[9] = tx; o.h[10] = ty; o.h[11] = tz;
    }
    o.z = -(double)pd2;
    if (NOISE) {
      const double a2 = o.h[0] * o.h[0] + o.h[1] * o.h[1] + o.h[2] * o.h[2];
      const double u = tx * ix + ty * iy + tz * iz;
      const double r2 = ix * ix + iy * iy + iz * iz;
      const double radial = r2 > 0.0 ? na.sr2 * (u * u) / r2 : 0.0;
      w = 1.0 / (na.base + radial + na.s2 * a2);
    }
  }
}

}  // namespace lii
