// Eigenvalues and eigenvectors of a symmetric 3 x 3 matrix in double, ONE routine for the host and the device (lii_sym3_eigen; the
// surface statistics of lii_surface.hip).  Cyclic Jacobi: kEig3Sweeps sweeps over the three off-diagonal entries, each annihilated by
// one plane rotation (Rutishauser's form: t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)), the diagonal moves by t * a_pq).  Every loop
// has a bound known before it starts - nothing waits for a residual to fall.
// Why not the closed form (trigonometric roots of the characteristic polynomial): it delivers every eigenvalue with an ABSOLUTE error of
// a few ulps of the largest one times a condition number of its own (the acos near +-1), and the small eigenvalue of a near-planar
// neighbourhood - the quantity the surface statistics exist for - drowns in it.  Jacobi's error is a few ulps of the largest eigenvalue,
// no more, and on a diagonal matrix it is none at all (no rotation is made).
// Sweep count: Jacobi converges quadratically once the off-diagonal mass is small; a 3 x 3 matrix is there after three sweeps at the
// latest and at rounding level after five (tests/test_sym3_eigen.py measures the residual over 10 000 covariances and the degenerate
// shapes).  Eight are made: the last ones find off-diagonal entries that are zero or negligible and make no rotation (eig3_rotate).
// Both forms must compute the same bits: the file is compiled without FMA contraction (-ffp-contract=off, csrc/Makefile), and it
// uses +, -, *, / and sqrt only - IEEE operations, rounded alike on both sides.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LII_EIG3_FN __host__ __device__ inline
#else
#define LII_EIG3_FN inline
#endif

namespace lii {

constexpr int kEig3Sweeps = 8;

// One rotation in the (p, q) plane of the matrix a (full symmetric storage) with the eigenvector columns v; r is the third index.
LII_EIG3_FN void eig3_rotate(double a[3][3], double v[3][3], int p, int q, int r) {
  const double apq = a[p][q];
  // an entry that is zero, or negligible beside its diagonal pair - |a_pq| <= 2^-53 sqrt(|a_pp a_qq|), the criterion that keeps the small
  // eigenvalues of a positive definite matrix to their own relative accuracy - is dropped without a rotation: the sweeps behind
  // convergence cost a comparison each (the solve runs on a single lane of the surface kernel, where its divisions are the bill)
  if (apq * apq <= 1.232595164407831e-32 * fabs(a[p][p] * a[q][q])) {  // 2^-106
    a[p][q] = 0.0;
    a[q][p] = 0.0;
    return;
  }
  const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
  // (theta^2 may overflow to +inf for a negligible a_pq: t = 0 then, and the entry is dropped, which is what its size deserves)
  const double at = fabs(theta) + sqrt(theta * theta + 1.0);
  const double t = theta < 0.0 ? -1.0 / at : 1.0 / at;
  const double c = 1.0 / sqrt(t * t + 1.0);
  const double s = t * c;
  const double tau = s / (1.0 + c);
  a[p][p] = a[p][p] - t * apq;
  a[q][q] = a[q][q] + t * apq;
  a[p][q] = 0.0;
  a[q][p] = 0.0;
  const double arp = a[r][p], arq = a[r][q];
  const double nrp = arp - s * (arq + tau * arp);
  const double nrq = arq + s * (arp - tau * arq);
  a[r][p] = nrp; a[p][r] = nrp;
  a[r][q] = nrq; a[q][r] = nrq;
  for (int k = 0; k < 3; k++) {
    const double vkp = v[k][p], vkq = v[k][q];
    v[k][p] = vkp - s * (vkq + tau * vkp);
    v[k][q] = vkq + s * (vkp - tau * vkq);
  }
}

LII_EIG3_FN void eig3_order(double e[3], double v[3][3], int i, int j) {
  if (e[j] < e[i]) {
    const double x = e[i]; e[i] = e[j]; e[j] = x;
    for (int k = 0; k < 3; k++) { const double y = v[k][i]; v[k][i] = v[k][j]; v[k][j] = y; }
  }
}

// m: xx, xy, xz, yy, yz, zz.  eig: ascending.  vec: row k = the unit eigenvector of eig[k] (the three rows are orthonormal).
// A NaN or infinite entry gives NaNs; nothing loops longer for it.
LII_EIG3_FN void sym3_eigen(const double m[6], double eig[3], double vec[9]) {
  double a[3][3] = {{m[0], m[1], m[2]}, {m[1], m[3], m[4]}, {m[2], m[4], m[5]}};
  double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
#pragma unroll
  for (int sweep = 0; sweep < kEig3Sweeps; sweep++) {
    eig3_rotate(a, v, 0, 1, 2);
    eig3_rotate(a, v, 0, 2, 1);
    eig3_rotate(a, v, 1, 2, 0);
  }
  double e[3] = {a[0][0], a[1][1], a[2][2]};
  // ascending, by three compare-exchanges of (value, column) with constant indices; equal values keep their order
  eig3_order(e, v, 0, 1);
  eig3_order(e, v, 1, 2);
  eig3_order(e, v, 0, 1);
  for (int k = 0; k < 3; k++) {
    eig[k] = e[k];
    vec[3 * k] = v[0][k];
    vec[3 * k + 1] = v[1][k];
    vec[3 * k + 2] = v[2][k];
  }
}

}  // namespace lii
