// esti_plane on the five neighbours of a point, as the units that fit planes share it: the fit launch of the registration pass (lii_fit.hip)
// and the pose scoring (lii_score.hip).  Device code only; double precision, contraction off (see Makefile) to track the CPU path.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace lii {

// ------------------------------------------------------------------------------------------------
// esti_plane<double> (include/common_lib.h:236-269): 5x3 least squares A n = -1 by column-pivoted
// Householder QR — Eigen's ColPivHouseholderQR algorithm (Eigen >= 3.3.4, third-party, restated from
// its published structure: max-norm column pivoting with LAPACK-WN-176 norm down-dating, reflectors,
// solve over nonzeroPivots).  Double precision, contraction off (see Makefile) to track the CPU path.
__device__ __forceinline__ void qr_solve_5x3(double (&a)[5][3], double (&x)[3]) {
  const double eps = 2.220446049250313e-16;
  double hc[3];
  int tr[3];
  double nu[3], nd[3];
  double maxn = 0;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    double s = 0;
#pragma unroll
    for (int r = 0; r < 5; r++) s += a[r][c] * a[r][c];
    nu[c] = nd[c] = sqrt(s);
    maxn = fmax(maxn, nu[c]);
  }
  const double th = maxn * eps;  // Eigen 3.3: threshold_helper = abs2(maxCoeff * epsilon) / rows
  const double thr_helper = th * th / 5.0;
  const double downdate_thr = 1.4901161193847656e-08;  // sqrt(eps)
  int nzp = 3;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    int big = k;
    double bigv = nu[k];
#pragma unroll
    for (int j = k + 1; j < 3; j++)
      if (nu[j] > bigv) { bigv = nu[j]; big = j; }
    if (nzp == 3 && bigv * bigv < thr_helper * (double)(5 - k)) nzp = k;
    tr[k] = big;
    if (big != k) {
#pragma unroll
      for (int j = k + 1; j < 3; j++)
        if (j == big) {
#pragma unroll
          for (int r = 0; r < 5; r++) { double t = a[r][k]; a[r][k] = a[r][j]; a[r][j] = t; }
          double t = nu[k]; nu[k] = nu[j]; nu[j] = t;
          t = nd[k]; nd[k] = nd[j]; nd[j] = t;
        }
    }
    double tail = 0;
#pragma unroll
    for (int r = k + 1; r < 5; r++) tail += a[r][k] * a[r][k];
    double c0 = a[k][k], beta, tau;
    if (tail <= 2.2250738585072014e-308) {
      tau = 0;
      beta = c0;
#pragma unroll
      for (int r = k + 1; r < 5; r++) a[r][k] = 0;
    } else {
      beta = sqrt(c0 * c0 + tail);
      if (c0 >= 0) beta = -beta;
      double den = c0 - beta;
#pragma unroll
      for (int r = k + 1; r < 5; r++) a[r][k] /= den;
      tau = (beta - c0) / beta;
    }
    hc[k] = tau;
    a[k][k] = beta;
    if (tau != 0) {
#pragma unroll
      for (int j = k + 1; j < 3; j++) {
        double tmp = a[k][j];
#pragma unroll
        for (int r = k + 1; r < 5; r++) tmp += a[r][k] * a[r][j];
        a[k][j] -= tau * tmp;
#pragma unroll
        for (int r = k + 1; r < 5; r++) a[r][j] -= tau * a[r][k] * tmp;
      }
    }
#pragma unroll
    for (int j = k + 1; j < 3; j++) {
      if (nu[j] != 0) {
        double t = fabs(a[k][j]) / nu[j];
        t = (1.0 + t) * (1.0 - t);
        t = t < 0 ? 0 : t;
        double ratio = nu[j] / nd[j];
        double t2 = t * ratio * ratio;
        if (t2 <= downdate_thr) {
          double s = 0;
#pragma unroll
          for (int r = k + 1; r < 5; r++) s += a[r][j] * a[r][j];
          nd[j] = sqrt(s);
          nu[j] = nd[j];
        } else {
          nu[j] *= sqrt(t);
        }
      }
    }
  }
  double c[5] = {-1.0, -1.0, -1.0, -1.0, -1.0};
#pragma unroll
  for (int k = 0; k < 3; k++) {
    if (k < nzp && hc[k] != 0) {
      double tmp = c[k];
#pragma unroll
      for (int r = k + 1; r < 5; r++) tmp += a[r][k] * c[r];
      c[k] -= hc[k] * tmp;
#pragma unroll
      for (int r = k + 1; r < 5; r++) c[r] -= hc[k] * a[r][k] * tmp;
    }
  }
  double y[3] = {0, 0, 0};
#pragma unroll
  for (int i = 2; i >= 0; i--) {
    if (i < nzp) {
      double s = c[i];
#pragma unroll
      for (int j = i + 1; j < 3; j++)
        if (j < nzp) s -= a[i][j] * y[j];
      y[i] = s / a[i][i];
    }
  }
  int perm[3] = {0, 1, 2};
#pragma unroll
  for (int k = 0; k < 3; k++) {
    // swap(perm[k], perm[tr[k]]) with tr[k] >= k, written without dynamic register indexing
#pragma unroll
    for (int j = k + 1; j < 3; j++)
      if (tr[k] == j) { int t = perm[k]; perm[k] = perm[j]; perm[j] = t; }
  }
  x[0] = x[1] = x[2] = 0;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    if (i < nzp) {
      double v = y[i];
      if (perm[i] == 0) x[0] = v;
      else if (perm[i] == 1) x[1] = v;
      else x[2] = v;
    }
  }
}

// esti_plane on 5 neighbours; returns validity and (n̂, d)
__device__ __forceinline__ bool fit_plane(const float4 (&nb)[5], double plane_thr, double& pa, double& pbn, double& pc,
                                          double& pd) {
  double a[5][3] = {{nb[0].x, nb[0].y, nb[0].z}, {nb[1].x, nb[1].y, nb[1].z}, {nb[2].x, nb[2].y, nb[2].z},
                    {nb[3].x, nb[3].y, nb[3].z}, {nb[4].x, nb[4].y, nb[4].z}};
  double nv[3];
  qr_solve_5x3(a, nv);
  double nn = sqrt(nv[0] * nv[0] + nv[1] * nv[1] + nv[2] * nv[2]);
  pa = nv[0] / nn; pbn = nv[1] / nn; pc = nv[2] / nn; pd = 1.0 / nn;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 5; j++)
    if (fabs(pa * nb[j].x + pbn * nb[j].y + pc * nb[j].z + pd) > plane_thr) ok = false;
  return ok;
}

// Equal squared distances inside the kept list are ordered by x, ascending — what the reference's heap comparator
// (PointType_CMP, include/ikd-Tree/ikd_Tree.h:50-61: ties within 1e-10 fall back to point.x) produces after
// Nearest_Search pops it.  (A tie across the 5th/6th place is resolved by visiting order in the tree and by
// cell order here; that case cannot be reproduced and is documented in DESIGN.md.)
__device__ __forceinline__ bool canon_ties(float4 (&nb)[5]) {
  if (!(nb[0].w == nb[1].w || nb[1].w == nb[2].w || nb[2].w == nb[3].w || nb[3].w == nb[4].w)) return false;  // the usual case
  bool changed = false;
#pragma unroll
  for (int pass = 0; pass < 4; pass++)
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (nb[j].w == nb[j + 1].w && nb[j].x > nb[j + 1].x) {
        float4 t = nb[j]; nb[j] = nb[j + 1]; nb[j + 1] = t;
        changed = true;
      }
  return changed;
}

}  // namespace lii
