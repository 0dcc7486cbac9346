// postproc.hip -- on-device pre/post-processing around the patch path:
//   * resampling between the image grid and the model-spacing grid      utils/image_tools.py:329-377 (sitk.Resample with
//     an identity transform, LINEAR / NN, default pixel value), called at core/seg_infer.py:267 and :330-333
//   * 26-connected component labelling of one label of a multi-label mask, component sizes, largest / size-thresholded
//     selection                                                            utils/image_tools.py:380-432
//   * bounding box of selected labels                                      utils/image_tools.py:481-510
// ITK semantics restated (no SimpleITK in this environment -> parity unpinned):
//   ResampleImageFilter: output index -> physical point -> continuous input index c (one affine map, evaluated in
//   double); inside test  -0.5 <= c < size - 0.5  per axis (ImageFunction::IsInsideBuffer), else the default pixel;
//   LinearInterpolateImageFunction clamps the 8-neighbourhood at the borders (a coordinate in [-0.5, 0) or
//   (size - 1, size - 0.5) takes the edge value); NearestNeighbor rounds half up.
//   Label maps also take 'LABEL_LINEAR' (not in the reference): every label's indicator interpolated linearly, as ITK's label
//   interpolators and batchgenerators' order-1 segmentation resampling do, and the arg-max over the labels (not the latter's
//   sequential `>= 0.5` overwrite), fused into one pass without the planes (resample_label_kernel below).
//   ConnectedComponentImageFilter(FullyConnected) + RelabelComponent: components ordered by size, ties by first
//   voxel in raster order -- the labels here are the component's smallest linear index, which gives the same order.
// All kernels are HBM-bound byte movers / integer work.
#include "seg3d_imagegrid.h"
#include "seg3d_bspline.h"
#include "label_device.h"
#include "mc_device.h"
#include "seg3d_hip.h"

// ---- elastic deformation of the sampled point (training augmentation) ----------------------
// c_src = M (i, 1) + L u(i'): u is a tensor-product cubic B-spline (millimetres, world axes) over a coarse control grid
// laid over the destination grid, i' the destination index with the axes of `mirror` reversed (so that a mirrored deformed
// crop is the flip of the plain one), L = diag(1 / s_src) D_src^-1.  Per axis of n voxels: t = i * (sp / h), k = floor(t),
// f = t - k, u = sum_j B_j(f) ctrl[k + j], uniform cubic basis.  Everything in double, like the affine map.
// DEFORM = false: an empty argument and no code -- the kernels below compile to what they were without the parameter.
template <bool DEFORM>
struct DeformArgs {};
template <>
struct DeformArgs<true> {
  double L[9];        // row-major 3 x 3
  double t[3];        // sp / h per axis (x, y, z)
  const float* ctrl;  // [gz][gy][gx][3] control displacements (x, y, z components), device
  int g[3];           // gx, gy, gz
  int mirror;         // bit 0 = x, 1 = y, 2 = z
};

// LDS image of a launch (dynamic shared memory): per destination index of every axis the four basis weights (doubles) and
// the first control index (they are constant along the other two axes, so they are computed once per workgroup, not per
// voxel), then the control grid, which every voxel of the launch shares.
struct DeformLds {
  const double* w;   // [Xo + Yo + Zo][4]
  const int* k;      // [Xo + Yo + Zo]
  const float* ctrl; // [gz][gy][gx][3]
};

static inline size_t deform_lds_bytes(int Xo, int Yo, int Zo, const int* g) {
  const size_t n = (size_t)Xo + Yo + Zo;
  return n * 4 * sizeof(double) + n * sizeof(int) + (size_t)g[0] * g[1] * g[2] * 3 * sizeof(float);
}

__device__ __forceinline__ DeformLds deform_stage(double* smem, const DeformArgs<true>& dfm, int Xo, int Yo, int Zo) {
  const int n = Xo + Yo + Zo;
  double* w = smem;
  int* k = reinterpret_cast<int*>(smem + 4 * n);
  float* c = reinterpret_cast<float*>(k + n);
  for (int e = threadIdx.x; e < n; e += blockDim.x) {
    const int a = e < Xo ? 0 : (e < Xo + Yo ? 1 : 2);
    const int i = e - (a == 0 ? 0 : (a == 1 ? Xo : Xo + Yo));
    const double t = i * dfm.t[a];
    double fl = floor(t);
    int kk = (int)fl;
    if (kk > dfm.g[a] - 4) kk = dfm.g[a] - 4;   // never taken for a grid the launcher accepted; keeps k + 3 < g regardless
    if (kk < 0) kk = 0;
    const double f = t - fl, f2 = f * f, f3 = f2 * f, o = 1.0 - f;
    w[4 * e + 0] = o * o * o / 6.0;
    w[4 * e + 1] = (3.0 * f3 - 6.0 * f2 + 4.0) / 6.0;
    w[4 * e + 2] = (-3.0 * f3 + 3.0 * f2 + 3.0 * f + 1.0) / 6.0;
    w[4 * e + 3] = f3 / 6.0;
    k[e] = kk;
  }
  const int nc = dfm.g[0] * dfm.g[1] * dfm.g[2] * 3;
  for (int e = threadIdx.x; e < nc; e += blockDim.x) c[e] = dfm.ctrl[e];
  __syncthreads();
  DeformLds l;
  l.w = w;
  l.k = k;
  l.ctrl = c;
  return l;
}

// adds L u(x', y', z') to the continuous source index (cx, cy, cz) of destination voxel (x, y, z)
__device__ __forceinline__ void deform_apply(const DeformLds& l, const DeformArgs<true>& dfm, int x, int y, int z, int Xo,
                                             int Yo, int Zo, double& cx, double& cy, double& cz) {
  const int ex = (dfm.mirror & 1) ? Xo - 1 - x : x;
  const int ey = Xo + ((dfm.mirror & 2) ? Yo - 1 - y : y);
  const int ez = Xo + Yo + ((dfm.mirror & 4) ? Zo - 1 - z : z);
  const int kx = l.k[ex], ky = l.k[ey], kz = l.k[ez];
  const double* wx = l.w + 4 * ex;
  const double* wy = l.w + 4 * ey;
  const double* wz = l.w + 4 * ez;
  const int gx = dfm.g[0], gy = dfm.g[1];
  double ux = 0.0, uy = 0.0, uz = 0.0;
#pragma unroll
  for (int jz = 0; jz < 4; ++jz) {
#pragma unroll
    for (int jy = 0; jy < 4; ++jy) {
      const float* row = l.ctrl + (((kz + jz) * gy + (ky + jy)) * gx + kx) * 3;
      const double wzy = wz[jz] * wy[jy];
#pragma unroll
      for (int jx = 0; jx < 4; ++jx) {
        const double wgt = wzy * wx[jx];
        ux += wgt * (double)row[3 * jx + 0];
        uy += wgt * (double)row[3 * jx + 1];
        uz += wgt * (double)row[3 * jx + 2];
      }
    }
  }
  cx += dfm.L[0] * ux + dfm.L[1] * uy + dfm.L[2] * uz;
  cy += dfm.L[3] * ux + dfm.L[4] * uy + dfm.L[5] * uz;
  cz += dfm.L[6] * ux + dfm.L[7] * uy + dfm.L[8] * uz;
}

// host side of the deform entries: checks and the by-value argument.  The control grid must cover every index the
// kernel reads (k + 3 with k = floor((n - 1) * sp / h), evaluated here with the device's own arithmetic) and the LDS image
// must fit the 64 KB a workgroup gets without opting in -- a training crop needs a few KB.
static int deform_args(const char* name, int Xo, int Yo, int Zo, const double* l_host, const float* ctrl, int gx, int gy,
                       int gz, const double* t_host, int mirror_mask, DeformArgs<true>* out) {
  SEG3D_REQUIRE(l_host && ctrl && t_host, "%s: null pointer", name);
  SEG3D_REQUIRE(mirror_mask >= 0 && mirror_mask <= 7, "%s: mirror mask %d outside 0..7", name, mirror_mask);
  const int n[3] = {Xo, Yo, Zo}, g[3] = {gx, gy, gz};
  for (int a = 0; a < 3; ++a) {
    SEG3D_REQUIRE(t_host[a] >= 0.0 && t_host[a] <= 1.0, "%s: spacing / grid factor %g of axis %d outside [0, 1]", name,
                  t_host[a], a);
    const double last = floor((n[a] - 1) * t_host[a]);
    SEG3D_REQUIRE(g[a] >= 4 && (double)g[a] >= last + 4.0 && g[a] <= 1024,
                  "%s: %d control points on axis %d, floor((n - 1) sp / h) + 4 = %.0f are needed", name, g[a], a, last + 4.0);
    out->t[a] = t_host[a];
    out->g[a] = g[a];
  }
  SEG3D_REQUIRE(deform_lds_bytes(Xo, Yo, Zo, g) <= 64 * 1024,
                "%s: weight tables + control grid need %zu bytes of LDS, 65536 are available (crop-sized grids only)", name,
                deform_lds_bytes(Xo, Yo, Zo, g));
  for (int k = 0; k < 9; ++k) out->L[k] = l_host[k];
  out->ctrl = ctrl;
  out->mirror = mirror_mask;
  return SEG3D_OK;
}

// ---- resampling: M co-registered channels in one pass (multi-modality training crops and inference resampling) --------
// src [Zi][Yi][Xi][M] (channels-last), dst: voxel (x, y, z) of the output grid at dst + ((z * Yo + y) * Xo + x) * dst_stride,
// M floats.  The affine coordinate, the inside test and the trilinear weights (or the NN index) are computed once per
// output voxel (trilinear_tap / trilinear_lerp of seg3d_imagegrid.h, shared with the ensemble accumulate); each of the 8
// taps is one contiguous M-float row.  Per channel the arithmetic is in double with one fixed operation order, clamping and
// padding whatever M is, so channel m of an M-channel launch equals the M = 1 launch on plane m bit for bit.  A single volume [Zi][Yi][Xi] is the M = 1, dst_stride = 1 case of the same memory:
// seg3d_resample_affine / seg3d_resample_deform are those entries.
// <MC, VEC>: the row width of the instantiation, mc_device.h.
// SRC: the element type of src -- float, or short / unsigned char / signed char for a volume kept as its file stores it
// (seg3d_resample_*_typed_mc).  Only the row loads know it: they convert each element with (float), which is exact for these
// types, so a typed launch equals the float launch on the converted volume bit for bit; dst is always fp32.
template <typename SRC, int MC, bool VEC, bool DEFORM>
__global__ __launch_bounds__(256) void resample_affine_mc_kernel(const SRC* __restrict__ src, float* __restrict__ dst,
                                                                   int Mrt, i64 dst_stride, int Xi, int Yi, int Zi, int Xo,
                                                                   int Yo, int Zo, Affine12 A, int linear, float pad,
                                                                   DeformArgs<DEFORM> dfm) {
  constexpr int MR = mc_regs<MC>;
  const int M = mc_width<MC>(Mrt);
  extern __shared__ double deform_smem[];
  DeformLds lds;
  if constexpr (DEFORM) lds = deform_stage(deform_smem, dfm, Xo, Yo, Zo);
  const i64 total = (i64)Xo * Yo * Zo;
  for (i64 idx = (i64)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (i64)gridDim.x * 256) {
    const int x = (int)(idx % Xo);
    const i64 t = idx / Xo;
    const int y = (int)(t % Yo), z = (int)(t / Yo);
    double cx, cy, cz;
    affine12_apply(A, x, y, z, cx, cy, cz);
    if constexpr (DEFORM) deform_apply(lds, dfm, x, y, z, Xo, Yo, Zo, cx, cy, cz);
    float out[MR];
#pragma unroll
    for (int m = 0; m < MR; ++m) out[m] = pad;
    if (SEG3D_INSIDE_BUFFER(cx, cy, cz, Xi, Yi, Zi)) {
      if (linear) {
        TrilinearTap tap;
        trilinear_tap(cx, cy, cz, Xi, Yi, Zi, tap);
        const double dx = tap.dx, dy = tap.dy, dz = tap.dz;
        const SRC *p000 = src + (tap.r00 + tap.x0) * M, *p100 = src + (tap.r00 + tap.x1) * M,
                  *p010 = src + (tap.r01 + tap.x0) * M, *p110 = src + (tap.r01 + tap.x1) * M,
                  *p001 = src + (tap.r10 + tap.x0) * M, *p101 = src + (tap.r10 + tap.x1) * M,
                  *p011 = src + (tap.r11 + tap.x0) * M, *p111 = src + (tap.r11 + tap.x1) * M;
        if constexpr (MC > 0) {
          float t000[MC], t100[MC], t010[MC], t110[MC], t001[MC], t101[MC], t011[MC], t111[MC];
          mc_load_row<MC, VEC>(p000, t000);
          mc_load_row<MC, VEC>(p100, t100);
          mc_load_row<MC, VEC>(p010, t010);
          mc_load_row<MC, VEC>(p110, t110);
          mc_load_row<MC, VEC>(p001, t001);
          mc_load_row<MC, VEC>(p101, t101);
          mc_load_row<MC, VEC>(p011, t011);
          mc_load_row<MC, VEC>(p111, t111);
#pragma unroll
          for (int m = 0; m < MC; ++m)
            out[m] = trilinear_lerp(t000[m], t100[m], t010[m], t110[m], t001[m], t101[m], t011[m], t111[m], dx, dy, dz);
        } else {   // the runtime width reads the eight rows channel by channel: as rows they would hold 64 registers
#pragma unroll
          for (int m = 0; m < MR; ++m)
            if (m < M)
              out[m] = trilinear_lerp(mc_load_elem(p000, m), mc_load_elem(p100, m), mc_load_elem(p010, m),
                                      mc_load_elem(p110, m), mc_load_elem(p001, m), mc_load_elem(p101, m),
                                      mc_load_elem(p011, m), mc_load_elem(p111, m), dx, dy, dz);
        }
      } else {
        int xn = (int)floor(cx + 0.5), yn = (int)floor(cy + 0.5), zn = (int)floor(cz + 0.5);
        xn = xn < 0 ? 0 : (xn >= Xi ? Xi - 1 : xn);
        yn = yn < 0 ? 0 : (yn >= Yi ? Yi - 1 : yn);
        zn = zn < 0 ? 0 : (zn >= Zi ? Zi - 1 : zn);
        mc_load_row<MC, VEC>(src + (((i64)zn * Yi + yn) * Xi + xn) * M, out, M, pad);
      }
    }
    mc_store_row<MC, VEC>(dst + idx * dst_stride, out, M);
  }
}

// MC_DISPATCH's callee: SRC and DEFORM come from the arguments.  Vector rows need the source base, the destination base
// and the destination stride aligned to the row width (mc_vec_rows_typed).
template <int MC, bool VEC, typename SRC, bool DEFORM>
static void resample_mc_launch(const SRC* src, float* dst, int M, i64 dst_stride, int Xi, int Yi, int Zi, int Xo, int Yo,
                               int Zo, const Affine12& A, int lin, float pad, const DeformArgs<DEFORM>& D, size_t lds,
                               hipStream_t s) {
  hipLaunchKernelGGL((resample_affine_mc_kernel<SRC, MC, VEC, DEFORM>), dim3(seg3d_ew_grid((i64)Xo * Yo * Zo, 256)), dim3(256),
                     lds, s, src, dst, M, dst_stride, Xi, Yi, Zi, Xo, Yo, Zo, A, lin, pad, D);
}

// the four entries' common checks and the by-value affine argument
static int resample_args(const char* name, const void* src, const float* dst, int M, long long dst_stride, int Xi, int Yi,
                         int Zi, int Xo, int Yo, int Zo, const double* affine_host, Affine12* A) {
  SEG3D_REQUIRE(src && dst && affine_host, "%s: null pointer", name);
  SEG3D_REQUIRE(M >= 1 && M <= 8, "%s: M = %d channels, 1..8 are supported", name, M);
  SEG3D_REQUIRE(dst_stride >= M, "%s: voxel stride %lld below M = %d", name, dst_stride, M);
  SEG3D_REQUIRE(Xi > 0 && Yi > 0 && Zi > 0 && Xo > 0 && Yo > 0 && Zo > 0, "%s: bad dims", name);
  for (int k = 0; k < 12; ++k) A->m[k] = affine_host[k];
  return SEG3D_OK;
}

// launch(T()) for the source element type T behind `src_dtype`, the codes of label_device.h: 0 int8, 1 uint8, 2 int16,
// 4 float32.  Code 3 (int32) is refused with the unknown codes: an int32 is not exact in a float.
template <typename F>
static inline int resample_src_dispatch(int src_dtype, const char* name, F&& launch) {
  switch (src_dtype) {
    case 0: launch((signed char)0); return SEG3D_OK;
    case 1: launch((unsigned char)0); return SEG3D_OK;
    case 2: launch((short)0); return SEG3D_OK;
    case 4: launch(0.0f); return SEG3D_OK;
    default:
      SEG3D_UNSUPPORTED("%s: source dtype code %d: 0 (int8), 1 (uint8), 2 (int16) and 4 (float32) are supported%s", name,
                        src_dtype, src_dtype == 3 ? "; an int32 is not exact in a float" : "");
  }
}

static int resample_affine(const char* name, const void* src, int src_dtype, float* dst, int M, long long dst_stride, int Xi,
                           int Yi, int Zi, int Xo, int Yo, int Zo, const double* affine_host, int linear, float pad,
                           void* stream) {
  Affine12 A;
  int rc = resample_args(name, src, dst, M, dst_stride, Xi, Yi, Zi, Xo, Yo, Zo, affine_host, &A);
  if (rc != SEG3D_OK) return rc;
  rc = resample_src_dispatch(src_dtype, name, [&](auto tag) {
    typedef decltype(tag) SRC;
    MC_DISPATCH(resample_mc_launch, M, mc_vec_rows_typed(M, src, sizeof(SRC), dst, dst_stride),
                ((const SRC*)src, dst, M, (i64)dst_stride, Xi, Yi, Zi, Xo, Yo, Zo, A, linear ? 1 : 0, pad, DeformArgs<false>(),
                 0, (hipStream_t)stream));
  });
  if (rc != SEG3D_OK) return rc;
  SEG3D_LAUNCH_CHECK(name);
  return SEG3D_OK;
}

static int resample_deform(const char* name, const void* src, int src_dtype, float* dst, int M, long long dst_stride, int Xi,
                           int Yi, int Zi, int Xo, int Yo, int Zo, const double* affine_host, int linear, float pad,
                           const double* l_host, const float* ctrl, int gx, int gy, int gz, const double* t_host,
                           int mirror_mask, void* stream) {
  Affine12 A;
  int rc = resample_args(name, src, dst, M, dst_stride, Xi, Yi, Zi, Xo, Yo, Zo, affine_host, &A);
  if (rc != SEG3D_OK) return rc;
  DeformArgs<true> D;
  rc = deform_args(name, Xo, Yo, Zo, l_host, ctrl, gx, gy, gz, t_host, mirror_mask, &D);
  if (rc != SEG3D_OK) return rc;
  rc = resample_src_dispatch(src_dtype, name, [&](auto tag) {
    typedef decltype(tag) SRC;
    MC_DISPATCH(resample_mc_launch, M, mc_vec_rows_typed(M, src, sizeof(SRC), dst, dst_stride),
                ((const SRC*)src, dst, M, (i64)dst_stride, Xi, Yi, Zi, Xo, Yo, Zo, A, linear ? 1 : 0, pad, D,
                 deform_lds_bytes(Xo, Yo, Zo, D.g), (hipStream_t)stream));
  });
  if (rc != SEG3D_OK) return rc;
  SEG3D_LAUNCH_CHECK(name);
  return SEG3D_OK;
}

// src [Zi][Yi][Xi][M] -> rows of M floats at dst + voxel * dst_stride (dst_stride >= M floats): dst = src sampled at
// c = M * (x, y, z, 1); affine_host: 12 doubles, row-major 3 x 4
extern "C" int seg3d_resample_affine_mc(const float* src, float* dst, int M, long long dst_stride, int Xi, int Yi, int Zi,
                                        int Xo, int Yo, int Zo, const double* affine_host, int linear, float pad,
                                        void* stream) {
  return resample_affine("seg3d_resample_affine_mc", src, 4, dst, M, dst_stride, Xi, Yi, Zi, Xo, Yo, Zo, affine_host, linear,
                         pad, stream);
}

// seg3d_resample_affine_mc with the sampled point displaced by a cubic B-spline field, one field for all M channels:
// c = M (x, y, z, 1) + L u(x', y', z')
extern "C" int seg3d_resample_deform_mc(const float* src, float* dst, int M, long long dst_stride, int Xi, int Yi, int Zi,
                                        int Xo, int Yo, int Zo, const double* affine_host, int linear, float pad,
                                        const double* l_host, const float* ctrl, int gx, int gy, int gz,
                                        const double* t_host, int mirror_mask, void* stream) {
  return resample_deform("seg3d_resample_deform_mc", src, 4, dst, M, dst_stride, Xi, Yi, Zi, Xo, Yo, Zo, affine_host, linear,
                         pad, l_host, ctrl, gx, gy, gz, t_host, mirror_mask, stream);
}

// the two entries above for a source of another element type: src_dtype 0 int8, 1 uint8, 2 int16, 4 float32 (the codes of
// label_device.h; 4 is the entry above); the row loads convert with (float), everything else is the same launch
extern "C" int seg3d_resample_affine_typed_mc(const void* src, int src_dtype, float* dst, int M, long long dst_stride, int Xi,
                                              int Yi, int Zi, int Xo, int Yo, int Zo, const double* affine_host, int linear,
                                              float pad, void* stream) {
  return resample_affine("seg3d_resample_affine_typed_mc", src, src_dtype, dst, M, dst_stride, Xi, Yi, Zi, Xo, Yo, Zo,
                         affine_host, linear, pad, stream);
}

extern "C" int seg3d_resample_deform_typed_mc(const void* src, int src_dtype, float* dst, int M, long long dst_stride, int Xi,
                                              int Yi, int Zi, int Xo, int Yo, int Zo, const double* affine_host, int linear,
                                              float pad, const double* l_host, const float* ctrl, int gx, int gy, int gz,
                                              const double* t_host, int mirror_mask, void* stream) {
  return resample_deform("seg3d_resample_deform_typed_mc", src, src_dtype, dst, M, dst_stride, Xi, Yi, Zi, Xo, Yo, Zo,
                         affine_host, linear, pad, l_host, ctrl, gx, gy, gz, t_host, mirror_mask, stream);
}

// the M = 1 case of the float entries above: src [Zi][Yi][Xi] -> dst [Zo][Yo][Xo]
extern "C" int seg3d_resample_affine(const float* src, float* dst, int Xi, int Yi, int Zi, int Xo, int Yo, int Zo,
                                     const double* affine_host, int linear, float pad, void* stream) {
  return resample_affine("seg3d_resample_affine", src, 4, dst, 1, 1, Xi, Yi, Zi, Xo, Yo, Zo, affine_host, linear, pad, stream);
}

extern "C" int seg3d_resample_deform(const float* src, float* dst, int Xi, int Yi, int Zi, int Xo, int Yo, int Zo,
                                     const double* affine_host, int linear, float pad, const double* l_host,
                                     const float* ctrl, int gx, int gy, int gz, const double* t_host, int mirror_mask,
                                     void* stream) {
  return resample_deform("seg3d_resample_deform", src, 4, dst, 1, 1, Xi, Yi, Zi, Xo, Yo, Zo, affine_host, linear, pad, l_host,
                         ctrl, gx, gy, gz, t_host, mirror_mask, stream);
}

// ---- cubic B-spline evaluation -----------------------------------------------------------
// The resampler above with the 64-tap spline of seg3d_bspline.h in place of the trilinear / NN branch: src holds the
// COEFFICIENTS of seg3d_bspline_prefilter_mc.  Index map, inside test, deformation, dst_stride and padding are the
// kernel's above (the same functions), so the geometry is the existing resampler's by construction.  A compile-time
// width gathers its 64 rows as rows (16 live at a time: one (z, y) line of four); the runtime width walks the channels
// one by one -- 64 rows of eight floats would not fit the register file.
template <int MC, bool VEC, bool DEFORM>
__global__ __launch_bounds__(256) void resample_bspline_mc_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                                    int Mrt, i64 dst_stride, int Xi, int Yi, int Zi, int Xo,
                                                                    int Yo, int Zo, Affine12 A, float pad,
                                                                    DeformArgs<DEFORM> dfm) {
  constexpr int MR = mc_regs<MC>;
  const int M = mc_width<MC>(Mrt);
  extern __shared__ double deform_smem[];
  DeformLds lds;
  if constexpr (DEFORM) lds = deform_stage(deform_smem, dfm, Xo, Yo, Zo);
  const i64 total = (i64)Xo * Yo * Zo;
  for (i64 idx = (i64)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (i64)gridDim.x * 256) {
    const int x = (int)(idx % Xo);
    const i64 t = idx / Xo;
    const int y = (int)(t % Yo), z = (int)(t / Yo);
    double cx, cy, cz;
    affine12_apply(A, x, y, z, cx, cy, cz);
    if constexpr (DEFORM) deform_apply(lds, dfm, x, y, z, Xo, Yo, Zo, cx, cy, cz);
    float out[MR];
#pragma unroll
    for (int m = 0; m < MR; ++m) out[m] = pad;
    if (SEG3D_INSIDE_BUFFER(cx, cy, cz, Xi, Yi, Zi)) {
      BsplineTap tap;
      bspline_tap(cx, cy, cz, Xi, Yi, Zi, tap);
      if constexpr (MC > 0) {
        bspline_eval<MC>(tap, Xi, Yi, [&](i64 voxel, float* v) { mc_load_row<MC, VEC>(src + voxel * MC, v); }, out);
      } else {
        for (int m = 0; m < M; ++m) {
          float o;
          bspline_eval<1>(tap, Xi, Yi, [&](i64 voxel, float* v) { v[0] = src[voxel * M + m]; }, &o);
#pragma unroll
          for (int k = 0; k < MR; ++k)   // static register index
            if (k == m) out[k] = o;
        }
      }
    }
    mc_store_row<MC, VEC>(dst + idx * dst_stride, out, M);
  }
}

template <int MC, bool VEC, bool DEFORM>
static void resample_bspline_mc_launch(const float* src, float* dst, int M, i64 dst_stride, int Xi, int Yi, int Zi, int Xo,
                                       int Yo, int Zo, const Affine12& A, float pad, const DeformArgs<DEFORM>& D, size_t lds,
                                       hipStream_t s) {
  hipLaunchKernelGGL((resample_bspline_mc_kernel<MC, VEC, DEFORM>), dim3(seg3d_ew_grid((i64)Xo * Yo * Zo, 256)), dim3(256),
                     lds, s, src, dst, M, dst_stride, Xi, Yi, Zi, Xo, Yo, Zo, A, pad, D);
}

static int resample_bspline(const char* name, const float* src, float* dst, int M, long long dst_stride, int Xi, int Yi,
                            int Zi, int Xo, int Yo, int Zo, const double* affine_host, float pad, void* stream) {
  Affine12 A;
  const int rc = resample_args(name, src, dst, M, dst_stride, Xi, Yi, Zi, Xo, Yo, Zo, affine_host, &A);
  if (rc != SEG3D_OK) return rc;
  MC_DISPATCH(resample_bspline_mc_launch, M, mc_vec_rows(M, src, dst, dst_stride),
              (src, dst, M, (i64)dst_stride, Xi, Yi, Zi, Xo, Yo, Zo, A, pad, DeformArgs<false>(), 0, (hipStream_t)stream));
  SEG3D_LAUNCH_CHECK(name);
  return SEG3D_OK;
}

static int resample_bspline_deform(const char* name, const float* src, float* dst, int M, long long dst_stride, int Xi,
                                   int Yi, int Zi, int Xo, int Yo, int Zo, const double* affine_host, float pad,
                                   const double* l_host, const float* ctrl, int gx, int gy, int gz, const double* t_host,
                                   int mirror_mask, void* stream) {
  Affine12 A;
  int rc = resample_args(name, src, dst, M, dst_stride, Xi, Yi, Zi, Xo, Yo, Zo, affine_host, &A);
  if (rc != SEG3D_OK) return rc;
  DeformArgs<true> D;
  rc = deform_args(name, Xo, Yo, Zo, l_host, ctrl, gx, gy, gz, t_host, mirror_mask, &D);
  if (rc != SEG3D_OK) return rc;
  MC_DISPATCH(resample_bspline_mc_launch, M, mc_vec_rows(M, src, dst, dst_stride),
              (src, dst, M, (i64)dst_stride, Xi, Yi, Zi, Xo, Yo, Zo, A, pad, D, deform_lds_bytes(Xo, Yo, Zo, D.g),
               (hipStream_t)stream));
  SEG3D_LAUNCH_CHECK(name);
  return SEG3D_OK;
}

// coefficients [Zi][Yi][Xi][M] -> rows of M floats at dst + voxel * dst_stride: the spline sampled at c = M * (x, y, z, 1)
extern "C" int seg3d_resample_bspline_mc(const float* src, float* dst, int M, long long dst_stride, int Xi, int Yi, int Zi,
                                         int Xo, int Yo, int Zo, const double* affine_host, float pad, void* stream) {
  return resample_bspline("seg3d_resample_bspline_mc", src, dst, M, dst_stride, Xi, Yi, Zi, Xo, Yo, Zo, affine_host, pad,
                          stream);
}

// seg3d_resample_bspline_mc with the sampled point displaced by the elastic field, c = M (x, y, z, 1) + L u(x', y', z')
extern "C" int seg3d_resample_bspline_deform_mc(const float* src, float* dst, int M, long long dst_stride, int Xi, int Yi,
                                                int Zi, int Xo, int Yo, int Zo, const double* affine_host, float pad,
                                                const double* l_host, const float* ctrl, int gx, int gy, int gz,
                                                const double* t_host, int mirror_mask, void* stream) {
  return resample_bspline_deform("seg3d_resample_bspline_deform_mc", src, dst, M, dst_stride, Xi, Yi, Zi, Xo, Yo, Zo,
                                 affine_host, pad, l_host, ctrl, gx, gy, gz, t_host, mirror_mask, stream);
}

// the M = 1 case of the two entries above: coefficients [Zi][Yi][Xi] -> dst [Zo][Yo][Xo]
extern "C" int seg3d_resample_bspline(const float* src, float* dst, int Xi, int Yi, int Zi, int Xo, int Yo, int Zo,
                                      const double* affine_host, float pad, void* stream) {
  return resample_bspline("seg3d_resample_bspline", src, dst, 1, 1, Xi, Yi, Zi, Xo, Yo, Zo, affine_host, pad, stream);
}

extern "C" int seg3d_resample_bspline_deform(const float* src, float* dst, int Xi, int Yi, int Zi, int Xo, int Yo, int Zo,
                                             const double* affine_host, float pad, const double* l_host, const float* ctrl,
                                             int gx, int gy, int gz, const double* t_host, int mirror_mask, void* stream) {
  return resample_bspline_deform("seg3d_resample_bspline_deform", src, dst, 1, 1, Xi, Yi, Zi, Xo, Yo, Zo, affine_host, pad,
                                 l_host, ctrl, gx, gy, gz, t_host, mirror_mask, stream);
}

// ---- per-label trilinear vote for label maps, 'LABEL_LINEAR'  ------------------------------
// The resampler above for one channel of LABELS: index map, deformation, inside test and the eight clamped taps are its own
// functions; in place of the lerp of the tap values stands label_linear_vote (seg3d_imagegrid.h) -- every distinct tap value's
// indicator is interpolated and the largest membership wins.  That is the arg-max over per-label 'LINEAR' planes without the
// planes: one launch of the size of the 'NN' launch, no workspace, no atomics.  A tap is converted with (float) like every
// typed element load and compared as a float; dst is fp32 as the 'NN' mask crop is.
template <typename SRC, bool DEFORM>
__global__ __launch_bounds__(256) void resample_label_kernel(const SRC* __restrict__ src, float* __restrict__ dst, int Xi,
                                                               int Yi, int Zi, int Xo, int Yo, int Zo, Affine12 A, float pad,
                                                               DeformArgs<DEFORM> dfm) {
  extern __shared__ double deform_smem[];
  DeformLds lds;
  if constexpr (DEFORM) lds = deform_stage(deform_smem, dfm, Xo, Yo, Zo);
  const i64 total = (i64)Xo * Yo * Zo;
  for (i64 idx = (i64)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (i64)gridDim.x * 256) {
    const int x = (int)(idx % Xo);
    const i64 t = idx / Xo;
    const int y = (int)(t % Yo), z = (int)(t / Yo);
    double cx, cy, cz;
    affine12_apply(A, x, y, z, cx, cy, cz);
    if constexpr (DEFORM) deform_apply(lds, dfm, x, y, z, Xo, Yo, Zo, cx, cy, cz);
    float out = pad;
    if (SEG3D_INSIDE_BUFFER(cx, cy, cz, Xi, Yi, Zi)) {
      TrilinearTap tap;
      trilinear_tap(cx, cy, cz, Xi, Yi, Zi, tap);
      out = label_linear_vote(mc_load_elem(src + tap.r00 + tap.x0, 0), mc_load_elem(src + tap.r00 + tap.x1, 0),
                              mc_load_elem(src + tap.r01 + tap.x0, 0), mc_load_elem(src + tap.r01 + tap.x1, 0),
                              mc_load_elem(src + tap.r10 + tap.x0, 0), mc_load_elem(src + tap.r10 + tap.x1, 0),
                              mc_load_elem(src + tap.r11 + tap.x0, 0), mc_load_elem(src + tap.r11 + tap.x1, 0), tap.dx,
                              tap.dy, tap.dz);
    }
    dst[idx] = out;
  }
}

template <bool DEFORM>
static int resample_label_launch(const char* name, const void* src, int src_dtype, float* dst, int Xi, int Yi, int Zi,
                                 int Xo, int Yo, int Zo, const Affine12& A, float pad, const DeformArgs<DEFORM>& D,
                                 size_t lds, void* stream) {
  const int rc = resample_src_dispatch(src_dtype, name, [&](auto tag) {
    typedef decltype(tag) SRC;
    hipLaunchKernelGGL((resample_label_kernel<SRC, DEFORM>), dim3(seg3d_ew_grid((i64)Xo * Yo * Zo, 256)), dim3(256), lds,
                       (hipStream_t)stream, (const SRC*)src, dst, Xi, Yi, Zi, Xo, Yo, Zo, A, pad, D);
  });
  if (rc != SEG3D_OK) return rc;
  SEG3D_LAUNCH_CHECK(name);
  return SEG3D_OK;
}

// label map src [Zi][Yi][Xi] of element type src_dtype (0 int8, 1 uint8, 2 int16, 4 float32) -> dst [Zo][Yo][Xo] fp32
extern "C" int seg3d_resample_label(const void* src, int src_dtype, float* dst, int Xi, int Yi, int Zi, int Xo, int Yo,
                                    int Zo, const double* affine_host, float pad, void* stream) {
  const char* name = "seg3d_resample_label";
  Affine12 A;
  const int rc = resample_args(name, src, dst, 1, 1, Xi, Yi, Zi, Xo, Yo, Zo, affine_host, &A);
  if (rc != SEG3D_OK) return rc;
  return resample_label_launch(name, src, src_dtype, dst, Xi, Yi, Zi, Xo, Yo, Zo, A, pad, DeformArgs<false>(), 0, stream);
}

// seg3d_resample_label with the sampled point displaced by the elastic field, c = M (x, y, z, 1) + L u(x', y', z')
extern "C" int seg3d_resample_label_deform(const void* src, int src_dtype, float* dst, int Xi, int Yi, int Zi, int Xo, int Yo,
                                           int Zo, const double* affine_host, float pad, const double* l_host,
                                           const float* ctrl, int gx, int gy, int gz, const double* t_host, int mirror_mask,
                                           void* stream) {
  const char* name = "seg3d_resample_label_deform";
  Affine12 A;
  int rc = resample_args(name, src, dst, 1, 1, Xi, Yi, Zi, Xo, Yo, Zo, affine_host, &A);
  if (rc != SEG3D_OK) return rc;
  DeformArgs<true> D;
  rc = deform_args(name, Xo, Yo, Zo, l_host, ctrl, gx, gy, gz, t_host, mirror_mask, &D);
  if (rc != SEG3D_OK) return rc;
  return resample_label_launch(name, src, src_dtype, dst, Xi, Yi, Zi, Xo, Yo, Zo, A, pad, D,
                               deform_lds_bytes(Xo, Yo, Zo, D.g), stream);
}

// ---- bounding box -----------------------------------------------------------------------------------------------------
struct LabelSet {
  int n;       // 0: every voxel > 0
  int v[16];
};

__global__ __launch_bounds__(256) void mask_bbox_kernel(const signed char* __restrict__ mask, int X, int Y, int Z, LabelSet ls,
                                                          int* __restrict__ box /* xmin ymin zmin xmax ymax zmax */) {
  LabelBox bx;
  const i64 total = (i64)X * Y * Z;
  for (i64 idx = (i64)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (i64)gridDim.x * 256) {
    const int m = mask[idx];
    bool sel = false;
    if (ls.n == 0) {
      sel = m > 0;
    } else {
#pragma unroll
      for (int k = 0; k < 16; ++k) sel = sel || (k < ls.n && m == ls.v[k]);
    }
    if (sel) {
      const int x = (int)(idx % X);
      const i64 t = idx / X;
      const int y = (int)(t % Y), z = (int)(t / Y);
      bx.add(x, y, z);
    }
  }
  bx.wave_commit(box);
}

// box_device[6] must be initialised to {INT_MAX x3, -1 x3}; afterwards (xmin, ymin, zmin, xmax, ymax, zmax) inclusive, or
// untouched when no voxel is selected.  nlabels == 0 selects every voxel > 0 (get_bounding_box(mask, None)).
extern "C" int seg3d_mask_bounding_box(const signed char* mask, int X, int Y, int Z, const int* labels_host, int nlabels,
                                       int* box_device, void* stream) {
  SEG3D_REQUIRE(mask && box_device && X > 0 && Y > 0 && Z > 0, "seg3d_mask_bounding_box: bad arguments");
  SEG3D_REQUIRE(nlabels >= 0 && nlabels <= 16 && (nlabels == 0 || labels_host), "seg3d_mask_bounding_box: 0..16 labels");
  LabelSet ls;
  ls.n = nlabels;
  for (int k = 0; k < 16; ++k) ls.v[k] = k < nlabels ? labels_host[k] : 0;
  i64 blocks = ((i64)X * Y * Z + 256 * 16 - 1) / (256 * 16);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(mask_bbox_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, mask, X, Y, Z, ls,
                     box_device);
  SEG3D_LAUNCH_CHECK("seg3d_mask_bounding_box");
  return SEG3D_OK;
}

// ---- 26-connected components of (mask == label) ----------------------------------------------------------------------
// Union-find on a parent array (label equivalence): parent[v] = v for foreground, -1 for background; every foreground
// voxel is merged with its 13 raster-predecessor neighbours (atomicMin on roots); a final pass flattens the trees, so a
// voxel's label is the smallest linear index of its component -- independent of the execution order.
__device__ __forceinline__ int ccl_find(const int* parent, int v) {
  int p = parent[v];
  while (p != v) {
    v = p;
    p = parent[v];
  }
  return v;
}

__device__ __forceinline__ void ccl_union(int* parent, int a, int b) {
  for (;;) {
    a = ccl_find(parent, a);
    b = ccl_find(parent, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(parent + a, b);  // a > b: hang the larger root under the smaller
    if (old == a) return;
    a = old;                                   // someone re-rooted a meanwhile: continue from there
  }
}

// foreground predicates of the two entries
struct CclEqual {
  int label;
  __device__ __forceinline__ bool operator()(int m) const { return m == label; }
};
struct CclNonZero {
  __device__ __forceinline__ bool operator()(int m) const { return m != 0; }
};

template <typename T, typename Pred>
__global__ __launch_bounds__(256) void ccl_init_kernel(const T* __restrict__ mask, Pred foreground, int* __restrict__ parent,
                                                         i64 total) {
  for (i64 idx = (i64)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (i64)gridDim.x * 256)
    parent[idx] = foreground(mask[idx]) ? (int)idx : -1;
}

__global__ __launch_bounds__(256) void ccl_merge_kernel(int* __restrict__ parent, int X, int Y, int Z) {
  const i64 total = (i64)X * Y * Z;
  for (i64 idx = (i64)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (i64)gridDim.x * 256) {
    if (parent[idx] < 0) continue;
    const int x = (int)(idx % X);
    const i64 t = idx / X;
    const int y = (int)(t % Y), z = (int)(t / Y);
    // the 13 neighbours that precede (x, y, z) in raster order
#pragma unroll
    for (int dz = -1; dz <= 0; ++dz)
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          if (dz == 0 && (dy > 0 || (dy == 0 && dx >= 0))) continue;
          const int xx = x + dx, yy = y + dy, zz = z + dz;
          if (xx < 0 || xx >= X || yy < 0 || yy >= Y || zz < 0) continue;
          const i64 u = ((i64)zz * Y + yy) * X + xx;
          if (parent[u] >= 0) ccl_union(parent, (int)idx, (int)u);
        }
  }
}

__global__ __launch_bounds__(256) void ccl_flatten_kernel(int* __restrict__ parent, i64 total) {
  for (i64 idx = (i64)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (i64)gridDim.x * 256)
    if (parent[idx] >= 0) parent[idx] = ccl_find(parent, (int)idx);
}

// parent = the flattened forest of the foreground of `mask`: every foreground voxel holds its component's lowest linear index
template <typename T, typename Pred>
static void ccl_forest(const T* mask, Pred foreground, int* parent, int X, int Y, int Z, hipStream_t s) {
  const i64 total = (i64)X * Y * Z;
  const dim3 grid(seg3d_ew_grid(total, 256));
  hipLaunchKernelGGL((ccl_init_kernel<T, Pred>), grid, dim3(256), 0, s, mask, foreground, parent, total);
  hipLaunchKernelGGL(ccl_merge_kernel, grid, dim3(256), 0, s, parent, X, Y, Z);
  hipLaunchKernelGGL(ccl_flatten_kernel, grid, dim3(256), 0, s, parent, total);
}

// sizes[id - first] += run length for the ids in first .. last, one atomic per run of equal ids among the consecutive voxels
// a thread walks: next(id) per voxel, flush() after the last.  Ids outside first .. last are counted nowhere.
struct CclRunAdd {
  int* sizes;
  int first, last;
  int cur = first - 1, run = 0;
  __device__ __forceinline__ void flush() {
    if (cur >= first && cur <= last) atomicAdd(sizes + (cur - first), run);
  }
  __device__ __forceinline__ void next(int id) {
    if (id != cur) {
      flush();
      cur = id;
      run = 0;
    }
    ++run;
  }
};

// sizes[root] += run length; a thread walks 32 consecutive voxels
__global__ __launch_bounds__(256) void ccl_count_kernel(const int* __restrict__ parent, int* __restrict__ sizes, i64 total) {
  const i64 base = ((i64)blockIdx.x * 256 + threadIdx.x) * 32;
  CclRunAdd runs{sizes, 0, INT_MAX};
  for (int k = 0; k < 32; ++k) {
    const i64 idx = base + k;
    runs.next(idx < total ? parent[idx] : -1);
  }
  runs.flush();
}

// best = max over roots of (size << 32 | ~root): the largest component, ties to the smallest root (first in raster order)
__global__ __launch_bounds__(256) void ccl_best_kernel(const int* __restrict__ parent, const int* __restrict__ sizes,
                                                         unsigned long long* __restrict__ best, i64 total) {
  unsigned long long key = 0ull;
  for (i64 idx = (i64)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (i64)gridDim.x * 256) {
    if (parent[idx] == (int)idx) {
      const unsigned long long k = ((unsigned long long)(unsigned)sizes[idx] << 32) | (0xffffffffull - (unsigned)idx);
      key = k > key ? k : key;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_down(key, off, 64);
    key = o > key ? o : key;
  }
  if ((threadIdx.x & 63) == 0 && key) atomicMax(best, key);
}

// out[v] = value where the voxel belongs to a kept component (mode 0: the largest; mode 1: size >= threshold);
// combine: 0 = overwrite (0 elsewhere), 1 = add `value` to the existing entry (multi-label composition)
__global__ __launch_bounds__(256) void ccl_select_kernel(const int* __restrict__ parent, const int* __restrict__ sizes,
                                                           const unsigned long long* __restrict__ best, int mode, int threshold,
                                                           signed char value, int combine, signed char* __restrict__ out,
                                                           i64 total) {
  const int best_root = (int)(0xffffffffull - (*best & 0xffffffffull));
  const bool any = *best != 0ull;
  for (i64 idx = (i64)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (i64)gridDim.x * 256) {
    const int r = parent[idx];
    bool keep = false;
    if (r >= 0) keep = mode == 0 ? (any && r == best_root) : sizes[r] >= threshold;
    const signed char v = keep ? value : (signed char)0;
    out[idx] = combine ? (signed char)(out[idx] + v) : v;
  }
}

extern "C" long long seg3d_ccl_workspace_ints(long long voxels) { return 2 * voxels + 2; }

// Components of (mask == label) with 26-connectivity; keeps the largest (mode 0) or those with >= threshold voxels
// (mode 1) and writes `value` there: out = (combine ? out : 0) + value * kept.  workspace: seg3d_ccl_workspace_ints ints.
extern "C" int seg3d_ccl26_select(const signed char* mask, int label, int X, int Y, int Z, int mode, int threshold, int value,
                                  int combine, signed char* out, int* workspace, void* stream) {
  SEG3D_REQUIRE(mask && out && workspace && X > 0 && Y > 0 && Z > 0, "seg3d_ccl26_select: bad arguments");
  SEG3D_REQUIRE((i64)X * Y * Z < (1ll << 31), "seg3d_ccl26_select: volume exceeds 2^31 voxels");
  SEG3D_REQUIRE(mode == 0 || mode == 1, "seg3d_ccl26_select: mode must be 0 (largest) or 1 (size threshold)");
  const i64 total = (i64)X * Y * Z;
  hipStream_t s = (hipStream_t)stream;
  int* parent = workspace;
  int* sizes = workspace + total;
  unsigned long long* best = reinterpret_cast<unsigned long long*>(workspace + 2 * total);  // 8-byte aligned: 2*total even
  const dim3 grid(seg3d_ew_grid(total, 256));
  if (hipMemsetAsync(sizes, 0, (size_t)(total + 2) * sizeof(int), s) != hipSuccess) {
    seg3d_set_error("seg3d_ccl26_select: hipMemsetAsync failed");
    return SEG3D_ERR_LAUNCH;
  }
  ccl_forest(mask, CclEqual{label}, parent, X, Y, Z, s);
  hipLaunchKernelGGL(ccl_count_kernel, dim3((unsigned)((total + 256 * 32 - 1) / (256 * 32))), dim3(256), 0, s, parent, sizes,
                     total);
  hipLaunchKernelGGL(ccl_best_kernel, grid, dim3(256), 0, s, parent, sizes, best, total);
  hipLaunchKernelGGL(ccl_select_kernel, grid, dim3(256), 0, s, parent, sizes, best, mode, threshold, (signed char)value,
                     combine, out, total);
  SEG3D_LAUNCH_CHECK("seg3d_ccl26_select");
  return SEG3D_OK;
}

// ---- 26-connected components of a 0/1 mask as a canonical id map (lesion-wise evaluation) ----
// ids doubles as the parent array of the union-find above (init / merge / flatten).  ccl_union only ever hangs a root
// under a SMALLER index (atomicMin, and a lost link is re-united from the displaced parent), so a parent is always below
// its child and the root that flatten leaves is the lowest linear index of the component, whatever the launch order.
// Numbering the roots by their rank in linear order therefore gives ids 1..K in the order of each component's lowest
// voxel.  The rank is an exclusive prefix sum of the root flags in three launches: per-block counts (4096 voxels per
// block), one block scanning the counts in rounds of 256 with a carry, and the per-block apply; no workgroup waits on
// another.  A last pass maps every voxel to its root's rank and adds run lengths to the size histogram (integer atomics).
#define CCL_SCAN_PER_THREAD 16
#define CCL_SCAN_ITEMS (256 * CCL_SCAN_PER_THREAD)

// exclusive prefix of v over the 256 threads of the block (thread order); total: the block's sum.  wave_tot: 4 shared ints
__device__ __forceinline__ int ccl_block_scan(int v, int* wave_tot, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int u = __shfl_up(inc, off, 64);
    if (lane >= off) inc += u;
  }
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int t = wave_tot[w];
    base += w < wave ? t : 0;
    total += t;
  }
  __syncthreads();   // wave_tot is free for the caller's next round
  return base + inc - v;
}

// thread t of block b owns the CCL_SCAN_PER_THREAD consecutive voxels from (b * 256 + t) * CCL_SCAN_PER_THREAD on;
// bit k of the result: voxel k of them is a root
__device__ __forceinline__ unsigned ccl_thread_roots(const int* __restrict__ parent, i64 first, i64 total) {
  unsigned bits = 0u;
#pragma unroll
  for (int k = 0; k < CCL_SCAN_PER_THREAD; ++k) {
    const i64 idx = first + k;
    if (idx < total && parent[idx] == (int)idx) bits |= 1u << k;
  }
  return bits;
}

__global__ __launch_bounds__(256) void ccl_root_sums_kernel(const int* __restrict__ parent, i64 total, int* __restrict__ sums) {
  __shared__ int wave_tot[4];
  const i64 first = ((i64)blockIdx.x * 256 + threadIdx.x) * CCL_SCAN_PER_THREAD;
  int block_total;
  ccl_block_scan(__popc(ccl_thread_roots(parent, first, total)), wave_tot, block_total);
  if (threadIdx.x == 0) sums[blockIdx.x] = block_total;
}

// one block: sums -> their exclusive prefix, count[0] = K, count[1] = (K > capacity); nblocks / 256 rounds
__global__ __launch_bounds__(256) void ccl_scan_sums_kernel(int* __restrict__ sums, int nblocks, int capacity,
                                                              int* __restrict__ count) {
  __shared__ int wave_tot[4];
  int carry = 0;
  for (int c0 = 0; c0 < nblocks; c0 += 256) {
    const int c = c0 + (int)threadIdx.x;
    const int v = c < nblocks ? sums[c] : 0;
    int round_total;
    const int ex = ccl_block_scan(v, wave_tot, round_total);
    if (c < nblocks) sums[c] = carry + ex;
    carry += round_total;
  }
  if (threadIdx.x == 0) {
    count[0] = carry;
    count[1] = carry > capacity ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void ccl_rank_apply_kernel(const int* __restrict__ parent, i64 total,
                                                               const int* __restrict__ sums, int* __restrict__ rank) {
  __shared__ int wave_tot[4];
  const i64 first = ((i64)blockIdx.x * 256 + threadIdx.x) * CCL_SCAN_PER_THREAD;
  const unsigned bits = ccl_thread_roots(parent, first, total);
  int block_total;
  int id = sums[blockIdx.x] + ccl_block_scan(__popc(bits), wave_tot, block_total);
#pragma unroll
  for (int k = 0; k < CCL_SCAN_PER_THREAD; ++k)
    if ((bits >> k) & 1u) rank[first + k] = ++id;   // bit k set implies first + k < total
}

// ids[v] = rank of v's root (0 on the background), in place over the parent array: a thread reads only its own
// parent words and the rank array.  sizes[id - 1] += run length for ids within the capacity.
__global__ __launch_bounds__(256) void ccl_relabel_kernel(int* __restrict__ ids, const int* __restrict__ rank, i64 total,
                                                            int* __restrict__ sizes, int capacity) {
  const i64 first = ((i64)blockIdx.x * 256 + threadIdx.x) * CCL_SCAN_PER_THREAD;
  CclRunAdd runs{sizes, 1, capacity};
#pragma unroll
  for (int k = 0; k < CCL_SCAN_PER_THREAD; ++k) {
    const i64 idx = first + k;
    if (idx >= total) break;
    const int r = ids[idx];
    const int id = r >= 0 ? rank[r] : 0;
    ids[idx] = id;
    runs.next(id);
  }
  runs.flush();
}

static inline i64 ccl_scan_blocks(i64 voxels) { return (voxels + CCL_SCAN_ITEMS - 1) / CCL_SCAN_ITEMS; }

extern "C" long long seg3d_ccl26_label_workspace_ints(long long voxels) {
  if (voxels <= 0 || voxels >= (1ll << 31)) return -1;
  return voxels + ccl_scan_blocks(voxels);
}

extern "C" int seg3d_ccl26_label(const unsigned char* mask, int X, int Y, int Z, int* ids, int* count_device, int* sizes,
                                 int capacity, int* workspace, void* stream) {
  SEG3D_REQUIRE(mask && ids && count_device && workspace, "seg3d_ccl26_label: null pointer");
  SEG3D_REQUIRE(X > 0 && Y > 0 && Z > 0 && (i64)X * Y * Z < (1ll << 31),
                "seg3d_ccl26_label: bad volume size %d x %d x %d (1 .. 2^31 - 1 voxels)", X, Y, Z);
  SEG3D_REQUIRE(capacity >= 0 && (capacity == 0 || sizes), "seg3d_ccl26_label: capacity %d without a sizes array", capacity);
  const i64 total = (i64)X * Y * Z;
  hipStream_t s = (hipStream_t)stream;
  int* rank = workspace;
  int* sums = workspace + total;
  const int nblocks = (int)ccl_scan_blocks(total);
  if (capacity > 0 && hipMemsetAsync(sizes, 0, (size_t)capacity * sizeof(int), s) != hipSuccess) {
    seg3d_set_error("seg3d_ccl26_label: hipMemsetAsync failed");
    return SEG3D_ERR_LAUNCH;
  }
  ccl_forest(mask, CclNonZero{}, ids, X, Y, Z, s);
  hipLaunchKernelGGL(ccl_root_sums_kernel, dim3(nblocks), dim3(256), 0, s, (const int*)ids, total, sums);
  hipLaunchKernelGGL(ccl_scan_sums_kernel, dim3(1), dim3(256), 0, s, sums, nblocks, capacity, count_device);
  hipLaunchKernelGGL(ccl_rank_apply_kernel, dim3(nblocks), dim3(256), 0, s, (const int*)ids, total, (const int*)sums, rank);
  hipLaunchKernelGGL(ccl_relabel_kernel, dim3(nblocks), dim3(256), 0, s, ids, (const int*)rank, total, sizes, capacity);
  SEG3D_LAUNCH_CHECK("seg3d_ccl26_label");
  return SEG3D_OK;
}
