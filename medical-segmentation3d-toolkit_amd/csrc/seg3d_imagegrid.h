// seg3d_imagegrid.h -- the affine index map, the trilinear tap of one output voxel, the per-label vote over its eight taps
// (resample_label_kernel, postproc.hip) and the two label rules with the by-value
// region order: one copy for resample_affine_mc_kernel (postproc.hip), finalize_argmax_kernel / finalize_regions_kernel
// (patch.hip) and ensemble_accumulate_kernel (ensemble.hip), so that the accumulate interpolates as the resampler and
// labels as the finalize kernels by construction (-ffp-contract=off: one expression, one sequence of roundings).
#pragma once
#include "seg3d_common.h"

struct Affine12 {
  double m[12];  // c = M[:, :3] * (x, y, z) + M[:, 3], rows = (cx, cy, cz)
};

// The region labels by value, one byte each: label r = (r < 8 ? lo >> 8 r : hi >> 8 (r - 8)) & 0xff.  Bytes in two words
// instead of an array: a by-value array indexed with a runtime r would be copied to scratch.
struct RegionOrder {
  unsigned long long lo, hi;
};
// order_host: R <= 16 host ints in 1..127 (the masks are int8); `name` is the entry the error message speaks for
static inline int region_order_from_host(const char* name, const int* order_host, int R, RegionOrder* order) {
  order->lo = order->hi = 0ull;
  for (int r = 0; r < R; ++r) {
    const int o = order_host[r];
    SEG3D_REQUIRE(o >= 1 && o <= 127, "%s: region_class_order[%d] = %d not in [1, 127]", name, r, o);
    if (r < 8)
      order->lo |= (unsigned long long)o << (8 * r);
    else
      order->hi |= (unsigned long long)o << (8 * (r - 8));
  }
  return SEG3D_OK;
}

#ifdef __HIPCC__
__device__ __forceinline__ int region_label(const RegionOrder& o, int r) {
  return (int)(((r < 8 ? o.lo >> (8 * r) : o.hi >> (8 * (r - 8)))) & 0xffull);
}

// arg-max, first maximum wins: class c takes over from the running (best, bv) only when strictly greater (never a NaN)
__device__ __forceinline__ void label_first_max(int c, float p, int& best, float& bv) {
  if (c == 0 || p > bv) best = c, bv = p;
}
// regions, sequential overwrite: visited for r = 0 .. R-1 in order from m = 0; p_r > 0.5 (strictly) writes `label`
__device__ __forceinline__ int label_region_overwrite(float p, int label, int m) { return p > 0.5f ? label : m; }

__device__ __forceinline__ void affine12_apply(const Affine12& A, int x, int y, int z, double& cx, double& cy, double& cz) {
  cx = A.m[0] * x + A.m[1] * y + A.m[2] * z + A.m[3];
  cy = A.m[4] * x + A.m[5] * y + A.m[6] * z + A.m[7];
  cz = A.m[8] * x + A.m[9] * y + A.m[10] * z + A.m[11];
}

struct TrilinearTap {      // what one output voxel needs from the geometry, shared by every channel / plane
  i64 r00, r01, r10, r11;  // row offsets (z0, y0), (z0, y1), (z1, y0), (z1, y1), in voxels of an [Zi][Yi][Xi] source
  int x0, x1;
  double dx, dy, dz;
};

// ITK's IsInsideBuffer, -0.5 <= c < size - 0.5 per axis.  A macro: inlined from a callee the chain costs a VGPR flag byte.
#define SEG3D_INSIDE_BUFFER(cx, cy, cz, Xi, Yi, Zi) \
  ((cx) >= -0.5 && (cx) < (Xi) - 0.5 && (cy) >= -0.5 && (cy) < (Yi) - 0.5 && (cz) >= -0.5 && (cz) < (Zi) - 0.5)

// Outside -- or for a NaN coordinate -- the clamps still give indices inside the source; the caller does not read them then.
__device__ __forceinline__ void trilinear_tap(double cx, double cy, double cz, int Xi, int Yi, int Zi, TrilinearTap& t) {
  const double fx = fmin(fmax(cx, 0.0), (double)(Xi - 1)), fy = fmin(fmax(cy, 0.0), (double)(Yi - 1)),
               fz = fmin(fmax(cz, 0.0), (double)(Zi - 1));
  const int x0 = (int)floor(fx), y0 = (int)floor(fy), z0 = (int)floor(fz);
  const int y1 = y0 + 1 < Yi ? y0 + 1 : y0, z1 = z0 + 1 < Zi ? z0 + 1 : z0;
  t.x0 = x0;
  t.x1 = x0 + 1 < Xi ? x0 + 1 : x0;
  t.dx = fx - x0, t.dy = fy - y0, t.dz = fz - z0;
  t.r00 = ((i64)z0 * Yi + y0) * Xi, t.r01 = ((i64)z0 * Yi + y1) * Xi;
  t.r10 = ((i64)z1 * Yi + y0) * Xi, t.r11 = ((i64)z1 * Yi + y1) * Xi;
}

// the eight corner values (v<x><y><z>) and the three weights, in double, one fixed operation order: x, then y, then z
__device__ __forceinline__ float trilinear_lerp(double v000, double v100, double v010, double v110, double v001, double v101,
                                                double v011, double v111, double dx, double dy, double dz) {
  const double a00 = v000 + (v100 - v000) * dx, a01 = v010 + (v110 - v010) * dx;
  const double a10 = v001 + (v101 - v001) * dx, a11 = v011 + (v111 - v011) * dx;
  const double b0 = a00 + (a01 - a00) * dy, b1 = a10 + (a11 - a10) * dy;
  return (float)(b0 + (b1 - b0) * dz);
}

// 'LABEL_LINEAR' (seg3d_resample_label): the eight tap VALUES of a label map, same corner
// order.  Every distinct value l is a candidate with the membership s_l = trilinear_lerp of its indicator (tap == l ? 1 : 0);
// the largest s_l wins, equal s_l go to the smallest l.  Candidates are enumerated in tap order -- a tap that repeats an
// earlier one is skipped -- with static selects only: no private array indexed at run time, so no scratch.  Eight equal taps
// return their value without a lerp: 1 + (1 - 1) d is exactly 1, the answer the general walk gives.
__device__ __forceinline__ float label_linear_vote(float t000, float t100, float t010, float t110, float t001, float t101,
                                                   float t011, float t111, double dx, double dy, double dz) {
  if (t100 == t000 && t010 == t000 && t110 == t000 && t001 == t000 && t101 == t000 && t011 == t000 && t111 == t000)
    return t000;
  float label = t000, best = -1.f;   // every s_l >= 0: the first candidate always takes over
  auto candidate = [&](float l, bool repeated) {
    if (repeated) return;
    const float s = trilinear_lerp(t000 == l ? 1.0 : 0.0, t100 == l ? 1.0 : 0.0, t010 == l ? 1.0 : 0.0,
                                   t110 == l ? 1.0 : 0.0, t001 == l ? 1.0 : 0.0, t101 == l ? 1.0 : 0.0,
                                   t011 == l ? 1.0 : 0.0, t111 == l ? 1.0 : 0.0, dx, dy, dz);
    if (s > best || (s == best && l < label)) best = s, label = l;
  };
  candidate(t000, false);
  candidate(t100, t100 == t000);
  candidate(t010, t010 == t000 || t010 == t100);
  candidate(t110, t110 == t000 || t110 == t100 || t110 == t010);
  candidate(t001, t001 == t000 || t001 == t100 || t001 == t010 || t001 == t110);
  candidate(t101, t101 == t000 || t101 == t100 || t101 == t010 || t101 == t110 || t101 == t001);
  candidate(t011, t011 == t000 || t011 == t100 || t011 == t010 || t011 == t110 || t011 == t001 || t011 == t101);
  candidate(t111, t111 == t000 || t111 == t100 || t111 == t010 || t111 == t110 || t111 == t001 || t111 == t101 ||
                      t111 == t011);
  return label;
}
#endif
