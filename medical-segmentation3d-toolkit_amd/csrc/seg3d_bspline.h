// seg3d_bspline.h -- the cubic B-spline tap of one output voxel (the definition is stated in
// include/seg3d_hip.h): tap indices with the whole-sample mirror, the uniform cubic basis weights and the summation order.
// One copy for resample_bspline_mc_kernel (postproc.hip) and for any later spline use on the image grid, as
// seg3d_imagegrid.h holds the trilinear tap (-ffp-contract=off: one expression, one sequence of roundings).
#pragma once
#include "seg3d_common.h"

// pole of the cubic B-spline prefilter, sqrt(3) - 2, and z / (z^2 - 1) of the anti-causal initialisation (= -z / (1 - z^2))
#define SEG3D_BSPLINE_POLE (-0.26794919243112270647)
#define SEG3D_BSPLINE_LAST (0.28867513459481288225)
// terms of the causal initialisation sum: |z|^24 = 1.9e-14
#define SEG3D_BSPLINE_HORIZON 24

// whole-sample mirror of any index onto 0 .. n-1 (d c b | a b c d | c b a): period 2 (n - 1), -1 -> 1, n -> n - 2; n = 1 -> 0
__host__ __device__ __forceinline__ int bspline_mirror(int i, int n) {
  if (n == 1) return 0;
  const int p = 2 * (n - 1);
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - i;
}

#ifdef __HIPCC__
struct BsplineTap {   // what one output voxel needs from the geometry, shared by every channel
  int x[4], y[4], z[4];          // mirrored indices of the taps k-1 .. k+2 per axis
  double wx[4], wy[4], wz[4];    // B_0 .. B_3(f)
};

// one axis: k = floor(c), f = c - k, taps k-1 .. k+2 mirrored, weights the uniform cubic basis (the elastic field's)
__device__ __forceinline__ void bspline_axis(double c, int n, int* idx, double* w) {
  const double fl = floor(c);
  const int k = (int)fl;
  const double f = c - fl, f2 = f * f, f3 = f2 * f, o = 1.0 - f;
  w[0] = o * o * o / 6.0;
  w[1] = (3.0 * f3 - 6.0 * f2 + 4.0) / 6.0;
  w[2] = (-3.0 * f3 + 3.0 * f2 + 3.0 * f + 1.0) / 6.0;
  w[3] = f3 / 6.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) idx[j] = bspline_mirror(k - 1 + j, n);
}

// the caller has checked SEG3D_INSIDE_BUFFER, so k is in -1 .. n-1 per axis
__device__ __forceinline__ void bspline_tap(double cx, double cy, double cz, int Xi, int Yi, int Zi, BsplineTap& t) {
  bspline_axis(cx, Xi, t.x, t.wx);
  bspline_axis(cy, Yi, t.y, t.wy);
  bspline_axis(cz, Zi, t.z, t.wz);
}

// out[0 .. N) = the spline of N channels at the tap: fetch(voxel, v) puts the N coefficients of source voxel
// (z * Yi + y) * Xi + x into v.  Double, one fixed order -- per (z, y) row the four x taps left to right, the four rows of a
// z plane, the four planes -- and one rounding to float.
template <int N, typename Fetch>
__device__ __forceinline__ void bspline_eval(const BsplineTap& t, int Xi, int Yi, Fetch fetch, float* out) {
  double r[N] = {};
  // the planes are a rolled loop (its index and weight picked by selects, not by a register-array index): unrolled, the
  // scheduler hoists all 64 row loads and a 4-wide row takes the whole register file (one wave per SIMD)
#pragma unroll 1
  for (int jz = 0; jz < 4; ++jz) {
    const int zi = jz == 0 ? t.z[0] : (jz == 1 ? t.z[1] : (jz == 2 ? t.z[2] : t.z[3]));
    const double wzj = jz == 0 ? t.wz[0] : (jz == 1 ? t.wz[1] : (jz == 2 ? t.wz[2] : t.wz[3]));
    double b[N];
#pragma unroll
    for (int jy = 0; jy < 4; ++jy) {
      const i64 row = ((i64)zi * Yi + t.y[jy]) * Xi;
      float v0[N], v1[N], v2[N], v3[N];
      fetch(row + t.x[0], v0);
      fetch(row + t.x[1], v1);
      fetch(row + t.x[2], v2);
      fetch(row + t.x[3], v3);
#pragma unroll
      for (int m = 0; m < N; ++m) {
        const double a = t.wx[0] * (double)v0[m] + t.wx[1] * (double)v1[m] + t.wx[2] * (double)v2[m] + t.wx[3] * (double)v3[m];
        b[m] = jy == 0 ? t.wy[0] * a : b[m] + t.wy[jy] * a;
      }
    }
#pragma unroll
    for (int m = 0; m < N; ++m) r[m] = jz == 0 ? wzj * b[m] : r[m] + wzj * b[m];
  }
#pragma unroll
  for (int m = 0; m < N; ++m) out[m] = (float)r[m];
}
#endif
