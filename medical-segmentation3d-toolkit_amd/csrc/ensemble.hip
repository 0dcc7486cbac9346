// ensemble.hip -- model ensembling on the image grid (not in the reference).
// The members of an ensemble may run at different spacings and strides, so their finalized probabilities can only be
// averaged on the image grid.  One launch per member: for every image voxel the source coordinate, the inside test and the
// trilinear weights are computed once and shared by the C planes; every plane is interpolated exactly as
// seg3d_resample_affine(linear = 1) does it (postproc.hip: same double-precision coordinate, same inside test
// -0.5 <= c < size - 0.5, same clamped 8-neighbourhood, same lerp order -- the library is built with -ffp-contract=off, so
// the same expressions give the same bits), multiplied by the member's weight and added into the image-grid accumulator;
// the launch of the last member writes the label map in the same pass (first-maximum arg-max, or the sequential region
// overwrite rule of finalize_regions_kernel).
// HBM-bound: the bytes are the accumulator planes (C * V * 4 read and written per member), moved 16 bytes per lane; the
// source taps are gathers from the (usually smaller) planar source and come from cache.  No LDS, no atomics, no scratch.
#include "seg3d_common.h"
#include "seg3d_hip.h"

#define ENSEMBLE_MAXC 16

struct EnsAffine {
  double m[12];  // c = M[:, :3] * (x, y, z) + M[:, 3], rows = (cx, cy, cz)
};

// the region labels by value, one byte each: label r = (r < 8 ? lo >> 8 r : hi >> 8 (r - 8)) & 0xff.  Bytes in two words
// instead of an array: the generic kernel indexes them with a runtime r, and a by-value array indexed at run time would be
// copied to scratch.
struct EnsOrder {
  unsigned long long lo, hi;
};
__device__ __forceinline__ int ens_label(const EnsOrder& o, int r) {
  return (int)(((r < 8 ? o.lo >> (8 * r) : o.hi >> (8 * (r - 8)))) & 0xffull);
}

// what one output voxel needs from the geometry: computed once, used by every plane
struct EnsTap {
  i64 r00, r01, r10, r11;  // row offsets (z0, y0), (z0, y1), (z1, y0), (z1, y1) inside a source plane
  int x0, x1;
  double dx, dy, dz;
  bool inside;
};

__device__ __forceinline__ void ens_tap(const EnsAffine& A, int x, int y, int z, int Xi, int Yi, int Zi, EnsTap& t) {
  const double cx = A.m[0] * x + A.m[1] * y + A.m[2] * z + A.m[3];
  const double cy = A.m[4] * x + A.m[5] * y + A.m[6] * z + A.m[7];
  const double cz = A.m[8] * x + A.m[9] * y + A.m[10] * z + A.m[11];
  t.inside = cx >= -0.5 && cx < Xi - 0.5 && cy >= -0.5 && cy < Yi - 0.5 && cz >= -0.5 && cz < Zi - 0.5;
  // (outside -- or a NaN coordinate -- the clamps below still give indices inside the source; they are not read then)
  const double fx = fmin(fmax(cx, 0.0), (double)(Xi - 1)), fy = fmin(fmax(cy, 0.0), (double)(Yi - 1)),
               fz = fmin(fmax(cz, 0.0), (double)(Zi - 1));
  const int x0 = (int)floor(fx), y0 = (int)floor(fy), z0 = (int)floor(fz);
  const int y1 = y0 + 1 < Yi ? y0 + 1 : y0, z1 = z0 + 1 < Zi ? z0 + 1 : z0;
  t.x0 = x0;
  t.x1 = x0 + 1 < Xi ? x0 + 1 : x0;
  t.dx = fx - x0;
  t.dy = fy - y0;
  t.dz = fz - z0;
  t.r00 = ((i64)z0 * Yi + y0) * Xi;
  t.r01 = ((i64)z0 * Yi + y1) * Xi;
  t.r10 = ((i64)z1 * Yi + y0) * Xi;
  t.r11 = ((i64)z1 * Yi + y1) * Xi;
}

// resample_mc_lerp of postproc.hip on one planar source
__device__ __forceinline__ float ens_lerp(const float* __restrict__ p, const EnsTap& t) {
  const double v000 = p[t.r00 + t.x0], v100 = p[t.r00 + t.x1], v010 = p[t.r01 + t.x0], v110 = p[t.r01 + t.x1];
  const double v001 = p[t.r10 + t.x0], v101 = p[t.r10 + t.x1], v011 = p[t.r11 + t.x0], v111 = p[t.r11 + t.x1];
  const double a00 = v000 + (v100 - v000) * t.dx, a01 = v010 + (v110 - v010) * t.dx;
  const double a10 = v001 + (v101 - v001) * t.dx, a11 = v011 + (v111 - v011) * t.dx;
  const double b0 = a00 + (a01 - a00) * t.dy, b1 = a10 + (a11 - a10) * t.dy;
  return (float)(b0 + (b1 - b0) * t.dz);
}

// CT = 1 .. 5: the class loop is compiled for exactly CT planes; CT = 0: runtime C <= 16.
// VEC: one thread owns 4 consecutive x of one output row (Xo % 4 == 0, acc 16-byte and mask 4-byte aligned): one 16-byte
// load and store per plane, one 4-byte mask store; otherwise one voxel per thread.
// FIRST: acc is not read.  mode 0: no mask; 1: arg-max (first maximum wins); 2: region overwrite rule.
template <int CT, bool VEC, bool FIRST>
__global__ __launch_bounds__(256) void ensemble_accumulate_kernel(const float* __restrict__ src, float* __restrict__ acc,
                                                                    signed char* __restrict__ mask, int Crt, int Xi, int Yi,
                                                                    int Zi, int Xo, int Yo, int Zo, EnsAffine A, float weight,
                                                                    float pad0, int mode, EnsOrder order) {
  constexpr int W = VEC ? 4 : 1;
  constexpr int UNROLL = CT > 0 ? CT : 1;   // the generic form keeps a runtime loop over its planes
  const int C = CT > 0 ? CT : Crt;
  const int Xq = Xo / W;
  const i64 items = (i64)Xq * Yo * Zo;
  const i64 vin = (i64)Xi * Yi * Zi, vout = (i64)Xo * Yo * Zo;
  for (i64 it = (i64)blockIdx.x * 256 + threadIdx.x; it < items; it += (i64)gridDim.x * 256) {
    const int xq = (int)(it % Xq);
    const i64 row = it / Xq;
    const int y = (int)(row % Yo), z = (int)(row / Yo);
    const i64 v0 = it * W;  // = (z * Yo + y) * Xo + xq * W
    EnsTap tap[W];
#pragma unroll
    for (int j = 0; j < W; ++j) ens_tap(A, xq * W + j, y, z, Xi, Yi, Zi, tap[j]);
    int lab[W];
    float bv[W];
#pragma unroll
    for (int j = 0; j < W; ++j) {
      lab[j] = 0;
      bv[j] = 0.f;
    }
#pragma unroll UNROLL
    for (int c = 0; c < C; ++c) {
      float* q = acc + (i64)c * vout + v0;
      float a[W];
      if constexpr (!FIRST) {
        if constexpr (VEC) {
          const float4 t4 = *reinterpret_cast<const float4*>(q);
          a[0] = t4.x; a[1] = t4.y; a[2] = t4.z; a[3] = t4.w;
        } else {
          a[0] = *q;
        }
      }
      const float* sp = src + (i64)c * vin;
      const float pad = c == 0 ? pad0 : 0.f;
#pragma unroll
      for (int j = 0; j < W; ++j) {
        float s = pad;
        if (tap[j].inside) s = ens_lerp(sp, tap[j]);
        const float p = __fmul_rn(weight, s);   // one rounding for the product, one for the sum: never an FMA
        a[j] = FIRST ? p : __fadd_rn(a[j], p);
      }
      if constexpr (VEC) {
        *reinterpret_cast<float4*>(q) = make_float4(a[0], a[1], a[2], a[3]);
      } else {
        *q = a[0];
      }
      if (mode == 1) {
#pragma unroll
        for (int j = 0; j < W; ++j)
          if (c == 0 || a[j] > bv[j]) {
            lab[j] = c;
            bv[j] = a[j];
          }
      } else if (mode == 2) {
        const int label = ens_label(order, c);
#pragma unroll
        for (int j = 0; j < W; ++j) lab[j] = a[j] > 0.5f ? label : lab[j];
      }
    }
    if (mode != 0) {
      if constexpr (VEC) {
        *reinterpret_cast<unsigned*>(mask + v0) = (unsigned)(lab[0] & 0xff) | ((unsigned)(lab[1] & 0xff) << 8) |
                                                  ((unsigned)(lab[2] & 0xff) << 16) | ((unsigned)(lab[3] & 0xff) << 24);
      } else {
        mask[v0] = (signed char)lab[0];
      }
    }
  }
}

#define ENSEMBLE_LAUNCH(CT)                                                                                             \
  do {                                                                                                                  \
    if (vec && first)                                                                                                   \
      hipLaunchKernelGGL((ensemble_accumulate_kernel<CT, true, true>), grid, block, 0, s, src, acc, mask, C, Xi, Yi, Zi, \
                         Xo, Yo, Zo, A, weight, pad0, mode, order);                                                     \
    else if (vec)                                                                                                       \
      hipLaunchKernelGGL((ensemble_accumulate_kernel<CT, true, false>), grid, block, 0, s, src, acc, mask, C, Xi, Yi,   \
                         Zi, Xo, Yo, Zo, A, weight, pad0, mode, order);                                                 \
    else if (first)                                                                                                     \
      hipLaunchKernelGGL((ensemble_accumulate_kernel<CT, false, true>), grid, block, 0, s, src, acc, mask, C, Xi, Yi,   \
                         Zi, Xo, Yo, Zo, A, weight, pad0, mode, order);                                                 \
    else                                                                                                                \
      hipLaunchKernelGGL((ensemble_accumulate_kernel<CT, false, false>), grid, block, 0, s, src, acc, mask, C, Xi, Yi,  \
                         Zi, Xo, Yo, Zo, A, weight, pad0, mode, order);                                                 \
  } while (0)

extern "C" int seg3d_ensemble_accumulate(const float* src, float* acc, signed char* mask, int C, int Xi, int Yi, int Zi,
                                         int Xo, int Yo, int Zo, const double* affine_host, float weight, int first,
                                         float pad0, const int* order_host, void* stream) {
  SEG3D_REQUIRE(src && acc && affine_host, "seg3d_ensemble_accumulate: null pointer");
  SEG3D_REQUIRE(C >= 1 && C <= ENSEMBLE_MAXC, "seg3d_ensemble_accumulate: %d planes not in [1, %d]", C, ENSEMBLE_MAXC);
  SEG3D_REQUIRE(Xi > 0 && Yi > 0 && Zi > 0 && Xo > 0 && Yo > 0 && Zo > 0, "seg3d_ensemble_accumulate: bad dims");
  EnsOrder order = {0ull, 0ull};
  if (order_host) {
    for (int r = 0; r < C; ++r) {
      const int o = order_host[r];
      SEG3D_REQUIRE(o >= 1 && o <= 127, "seg3d_ensemble_accumulate: region_class_order[%d] = %d not in [1, 127]", r, o);
      if (r < 8)
        order.lo |= (unsigned long long)o << (8 * r);
      else
        order.hi |= (unsigned long long)o << (8 * (r - 8));
    }
  }
  EnsAffine A;
  for (int k = 0; k < 12; ++k) A.m[k] = affine_host[k];
  const int mode = mask ? (order_host ? 2 : 1) : 0;
  // 16-byte rows: every plane of acc starts 16-byte aligned when the base is and Xo % 4 == 0 (the plane is a multiple of 4)
  const bool vec = Xo % 4 == 0 && ((uintptr_t)acc & 15) == 0 && ((uintptr_t)mask & 3) == 0;
  const i64 items = (i64)(vec ? Xo / 4 : Xo) * Yo * Zo;
  const dim3 grid(seg3d_ew_grid(items, 256)), block(256);
  hipStream_t s = (hipStream_t)stream;
  switch (C) {
    case 1: ENSEMBLE_LAUNCH(1); break;
    case 2: ENSEMBLE_LAUNCH(2); break;
    case 3: ENSEMBLE_LAUNCH(3); break;
    case 4: ENSEMBLE_LAUNCH(4); break;
    case 5: ENSEMBLE_LAUNCH(5); break;
    default: ENSEMBLE_LAUNCH(0); break;
  }
  SEG3D_LAUNCH_CHECK("seg3d_ensemble_accumulate");
  return SEG3D_OK;
}
