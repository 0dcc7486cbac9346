// ensemble.hip -- the image-grid tail of inference (not in the reference).
// A model's finalized probabilities live on the model's grid (its own spacing, sized to its stride); one launch per member
// brings all C planes to the image grid, multiplies them by the member's weight and adds them into the image-grid
// accumulator, and the launch of the last member writes the label map in the same pass.  A single model is the K = 1 case:
// weight 1.0f (w * s == s exactly) and `first`, so the accumulator is never read and leaves as the resampled planes.
// Per image voxel the tap is computed once and shared by the C planes; tap, lerp and label rules are the resampler's and
// the finalize kernels' own (seg3d_imagegrid.h): every plane equals seg3d_resample_affine(linear = 1) bit for bit.
// HBM-bound: the bytes are the accumulator planes (C * V * 4 read and written per member), moved 16 bytes per lane; the
// source taps are gathers from the (usually smaller) planar source and come from cache.  No LDS, no atomics, no scratch.
#include "seg3d_imagegrid.h"
#include "seg3d_hip.h"

#define ENSEMBLE_MAXC 16

// trilinear_lerp on one planar source
__device__ __forceinline__ float ens_plane(const float* __restrict__ p, const TrilinearTap& t) {
  return trilinear_lerp(p[t.r00 + t.x0], p[t.r00 + t.x1], p[t.r01 + t.x0], p[t.r01 + t.x1], p[t.r10 + t.x0], p[t.r10 + t.x1],
                        p[t.r11 + t.x0], p[t.r11 + t.x1], t.dx, t.dy, t.dz);
}

// CT = 1 .. 5: the class loop is compiled for exactly CT planes; CT = 0: runtime C <= 16.
// VEC: one thread owns 4 consecutive x of one output row (Xo % 4 == 0, acc 16-byte and mask 4-byte aligned): one 16-byte
// load and store per plane, one 4-byte mask store; otherwise one voxel per thread.
// FIRST: acc is not read.  mode 0: no mask; 1: arg-max (first maximum wins); 2: region overwrite rule.
template <int CT, bool VEC, bool FIRST>
__global__ __launch_bounds__(256) void ensemble_accumulate_kernel(const float* __restrict__ src, float* __restrict__ acc,
                                                                    signed char* __restrict__ mask, int Crt, int Xi, int Yi,
                                                                    int Zi, int Xo, int Yo, int Zo, Affine12 A, float weight,
                                                                    float pad0, int mode, RegionOrder order) {
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
    TrilinearTap tap[W];
    bool inside[W];
#pragma unroll
    for (int j = 0; j < W; ++j) {
      double cx, cy, cz;
      affine12_apply(A, xq * W + j, y, z, cx, cy, cz);
      inside[j] = SEG3D_INSIDE_BUFFER(cx, cy, cz, Xi, Yi, Zi);
      trilinear_tap(cx, cy, cz, Xi, Yi, Zi, tap[j]);
    }
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
        if (inside[j]) s = ens_plane(sp, tap[j]);
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
        for (int j = 0; j < W; ++j) label_first_max(c, a[j], lab[j], bv[j]);
      } else if (mode == 2) {
        const int label = region_label(order, c);
#pragma unroll
        for (int j = 0; j < W; ++j) lab[j] = label_region_overwrite(a[j], label, lab[j]);
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
  RegionOrder order = {0ull, 0ull};
  if (order_host && region_order_from_host("seg3d_ensemble_accumulate", order_host, C, &order) != SEG3D_OK)
    return SEG3D_ERR_INVALID;
  Affine12 A;
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
