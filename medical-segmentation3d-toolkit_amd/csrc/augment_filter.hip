// augment_filter.hip -- the two stencil transforms of the training augmentation: Gaussian blur
// and low-resolution simulation of a normalised crop, out of place.  The crop is channels-last [z][y][x][M] (M = 1: planar).
// Both are pure functions of (crop, parameters, voxel, modality): the result does not depend on tiling, grid, M or
// alignment, so the vector-row and the scalar paths are bit-equal.  fp32, no FMA contraction (-ffp-contract=off).
// One workgroup of 256 threads per 8 x 8 x 32 (z, y, x) output tile; thread (y, x) owns the tile's z column of every
// channel in registers and writes it as whole voxel rows at the end.
//
// Blur (separable x, y, z; taps added in the order -R..R onto 0; half-sample reflection i' = i mod 2n, i' >= n -> 2n - 1 - i'):
//   the workgroup walks the 8 + 2R input planes of its tile.  A plane with its R-voxel (y, x) halo is staged in LDS for
//   all MC channels (reflected indices from small LDS tables, so every load is in bounds), filtered along x in LDS, along y
//   into a register, and that value is added, times its tap, to the at most 2R + 1 outputs of the thread's z column it
//   belongs to: the planes arrive in the order -R..R of every output, so the z pass needs no buffer.  Radii and taps are
//   workgroup-uniform: the x and y sums take them from the kernel arguments (scalar registers) and run one code path per
//   radius that issues all its LDS reads before the first add; the z taps come from a small LDS table.  The next plane's
//   rows are loaded into registers while the current one is filtered.  The crop is read once per tile (halo re-reads
//   come from the caches) and written once.  LDS: MC (8 + 2R)(64 + 2R) floats -- 15.7 KB for four channels at R = 3,
//   24 KB at R = 6: occupancy is bounded by the 32 waves of a CU and the registers, not by LDS.
//   MC = 4 / 2 with 16- / 8-byte rows when M = 4 / 2 and both bases are aligned, otherwise one channel per workgroup
//   (grid y = M) with scalar accesses of stride M.
// Low-resolution simulation (nearest down-sampling, Keys cubic a = -0.5 up-sampling, the low grid is never stored):
//   per modality the workgroup gathers the patch of low-grid voxels its tile needs (at most 11 x 11 x 35, each read from its
//   source voxel) into LDS and up-samples it there along x, y and z; per-axis patch offsets, tap bases and weights are
//   integer arithmetic done once per tile.  A modality whose three sizes equal the crop's is copied.
#include "mc_device.h"
#include "seg3d_hip.h"

#define FLT_TX 32
#define FLT_TY 8
#define FLT_TZ 8

__device__ __forceinline__ int filter_reflect(int i, int n) {
  const int p = 2 * n;
  int r = i % p;
  if (r < 0) r += p;
  return r >= n ? p - 1 - r : r;
}

__device__ __forceinline__ void filter_tile_origin(int tiles_x, int tiles_y, int& x0, int& y0, int& z0) {
  const int t = blockIdx.x;
  const int tz = t / (tiles_x * tiles_y), r = t - tz * (tiles_x * tiles_y);
  const int ty = r / tiles_x;
  x0 = (r - ty * tiles_x) * FLT_TX;
  y0 = ty * FLT_TY;
  z0 = tz * FLT_TZ;
}

// sum_{k = -RC..RC} w[|k|] p[k * stride], added left to right onto 0: all reads first, then the sum
template <int RC>
__device__ __forceinline__ float blur_taps_n(const float* p, int stride, const float (&w)[7]) {
  float v[2 * RC + 1];
#pragma unroll
  for (int t = 0; t <= 2 * RC; ++t) v[t] = p[(t - RC) * stride];
  float acc = 0.f;
#pragma unroll
  for (int t = 0; t <= 2 * RC; ++t) acc = acc + w[t < RC ? RC - t : t - RC] * v[t];
  return acc;
}

// the same for a workgroup-uniform radius rc = 0..6; rc = 0 passes p[0] through
__device__ __forceinline__ float blur_taps(const float* p, int stride, const float (&w)[7], int rc) {
  switch (rc) {
    case 1: return blur_taps_n<1>(p, stride, w);
    case 2: return blur_taps_n<2>(p, stride, w);
    case 3: return blur_taps_n<3>(p, stride, w);
    case 4: return blur_taps_n<4>(p, stride, w);
    case 5: return blur_taps_n<5>(p, stride, w);
    case 6: return blur_taps_n<6>(p, stride, w);
    default: return p[0];
  }
}

// floats of dynamic LDS of augment_blur_kernel<MC> at halo R
static size_t blur_lds_floats(int MC, int R) {
  const int PW = FLT_TX + 2 * R, PH = FLT_TY + 2 * R, PZ = FLT_TZ + 2 * R;
  return (size_t)MC * (PH * PW + PH * FLT_TX + 8) + PW + PH + PZ;
}

// channels [blockIdx.y * MC, +MC) of the tile blockIdx.x; R = the largest radius of any modality (the staged halo)
template <int MC, bool VEC>
__global__ __launch_bounds__(256) void augment_blur_kernel(const float* __restrict__ src, float* __restrict__ dst, int X, int Y,
                                                             int Z, int M, int R, int tiles_x, int tiles_y,
                                                             Seg3dBlurParams prm) {
  extern __shared__ __attribute__((aligned(16))) float blur_smem[];
  const int PW = FLT_TX + 2 * R, PH = FLT_TY + 2 * R, PZ = FLT_TZ + 2 * R;
  float* P = blur_smem;                              // [MC][PH][PW]  one input plane with its halo
  float* Q = P + MC * PH * PW;                       // [MC][PH][TX]  after the x pass
  float* WL = Q + MC * PH * FLT_TX;                  // [MC][8]  taps w[|k|], 0 past the channel's radius
  int* XR = reinterpret_cast<int*>(WL + MC * 8);     // [PW] [PH] [PZ]  reflected source indices
  int* YR = XR + PW;
  int* ZR = YR + PH;
  const int c0 = blockIdx.y * MC;
  int x0, y0, z0;
  filter_tile_origin(tiles_x, tiles_y, x0, y0, z0);
  const int tid = threadIdx.x;
  const int x = tid & (FLT_TX - 1), y = tid >> 5;
  for (int i = tid; i < PW; i += 256) XR[i] = filter_reflect(x0 - R + i, X);
  for (int i = tid; i < PH; i += 256) YR[i] = filter_reflect(y0 - R + i, Y);
  for (int i = tid; i < PZ; i += 256) ZR[i] = filter_reflect(z0 - R + i, Z);
  int rc[MC];
  float w[MC][7];
#pragma unroll
  for (int c = 0; c < MC; ++c) {
    rc[c] = prm.radius[c0 + c];
#pragma unroll
    for (int k = 0; k < 7; ++k) w[c][k] = prm.taps[c0 + c][k];
  }
  if (tid < MC * 8) {
    const int c = tid >> 3, k = tid & 7;
    WL[tid] = k <= prm.radius[c0 + c] ? prm.taps[c0 + c][k < 7 ? k : 6] : 0.f;
  }
  float out[FLT_TZ][MC];
#pragma unroll
  for (int o = 0; o < FLT_TZ; ++o)
#pragma unroll
    for (int c = 0; c < MC; ++c) out[o][c] = 0.f;
  // the rows of a plane a thread stages: item tid + 256 j of the (PH x PW) plane, at most BLUR_STAGE of them; the next
  // plane's rows are loaded into registers while the current plane is filtered
  constexpr int BLUR_STAGE = ((FLT_TY + 12) * (FLT_TX + 12) + 255) / 256;
  const float rpw = 1.0f / (float)PW;
  i64 soff[BLUR_STAGE];
#pragma unroll
  for (int j = 0; j < BLUR_STAGE; ++j) soff[j] = -1;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < BLUR_STAGE; ++j) {
    const int idx = tid + 256 * j;
    if (idx < PH * PW) {
      const int py = seg3d_fdiv(idx, rpw), px = idx - py * PW;
      soff[j] = ((i64)YR[py] * X + XR[px]) * M + c0;               // offset inside a z plane
    }
  }
  const i64 zstride = (i64)Y * X * M;
  float stage[BLUR_STAGE][MC];
#pragma unroll
  for (int j = 0; j < BLUR_STAGE; ++j)
    if (soff[j] >= 0) mc_load_row<MC, VEC>(src + ZR[0] * zstride + soff[j], stage[j]);

  for (int lz = 0; lz < PZ; ++lz) {
#pragma unroll
    for (int j = 0; j < BLUR_STAGE; ++j)
      if (soff[j] >= 0) {
#pragma unroll
        for (int c = 0; c < MC; ++c) P[c * PH * PW + tid + 256 * j] = stage[j][c];
      }
    __syncthreads();
    if (lz + 1 < PZ) {
      const float* next = src + ZR[lz + 1] * zstride;
#pragma unroll
      for (int j = 0; j < BLUR_STAGE; ++j)
        if (soff[j] >= 0) mc_load_row<MC, VEC>(next + soff[j], stage[j]);
    }
#pragma unroll
    for (int c = 0; c < MC; ++c)
      for (int idx = tid; idx < PH * FLT_TX; idx += 256)             // idx = py * TX + x
        Q[c * PH * FLT_TX + idx] = blur_taps(P + (c * PH + (idx >> 5)) * PW + (idx & (FLT_TX - 1)) + R, 1, w[c], rc[c]);
    __syncthreads();
    const int p = lz - R;                                            // the plane z0 + p
#pragma unroll
    for (int c = 0; c < MC; ++c) {
      const float v = blur_taps(Q + (c * PH + y + R) * FLT_TX + x, FLT_TX, w[c], rc[c]);
      if (rc[c] == 0) {
#pragma unroll
        for (int o = 0; o < FLT_TZ; ++o) out[o][c] = p == o ? v : out[o][c];
      } else {
        float wk[FLT_TZ];                                            // output z0 + o takes this plane with tap k = p - o
#pragma unroll
        for (int o = 0; o < FLT_TZ; ++o) {
          const int ak = p < o ? o - p : p - o;                      // workgroup-uniform
          wk[o] = WL[c * 8 + (ak < 7 ? ak : 7)];
        }
#pragma unroll
        for (int o = 0; o < FLT_TZ; ++o) {
          const int ak = p < o ? o - p : p - o;
          const float t = out[o][c] + wk[o] * v;
          out[o][c] = ak <= rc[c] ? t : out[o][c];
        }
      }
    }
  }
  if (x0 + x >= X || y0 + y >= Y) return;
#pragma unroll
  for (int o = 0; o < FLT_TZ; ++o)
    if (z0 + o < Z) mc_store_row<MC, VEC>(dst + (((i64)(z0 + o) * Y + (y0 + y)) * X + (x0 + x)) * M + c0, out[o]);
}

// low-grid index k of output index i (the taps are k - 1 .. k + 2): floor(((2 i + 1) n' - n) / 2n), >= -1
__device__ __forceinline__ int lowres_k(int i, int n, int nl) {
  const int num = (2 * i + 1) * nl - n;
  return num < 0 ? -1 : num / (2 * n);
}

// weights of output index i and its first tap's position in the patch that starts at low index kmin - 1
__device__ __forceinline__ void lowres_entry(int i, int n, int nl, int kmin, float* w, int* j) {
  const int k = lowres_k(i, n, nl);
  const float f = (float)((2 * i + 1) * nl - n - 2 * n * k) / (float)(2 * n);
  const float f2 = f * f, f3 = f2 * f;
  w[0] = -0.5f * f3 + f2 - 0.5f * f;
  w[1] = 1.5f * f3 - 2.5f * f2 + 1.0f;
  w[2] = -1.5f * f3 + 2.0f * f2 + 0.5f * f;
  w[3] = 0.5f * f3 - 0.5f * f2;
  *j = k - kmin;
}

// source index of patch position j: s(clamp(kmin - 1 + j, 0, n' - 1)), s(q) = min(n - 1, ((2 q + 1) n) / (2 n'))
__device__ __forceinline__ int lowres_source(int j, int n, int nl, int kmin) {
  int q = kmin - 1 + j;
  q = q < 0 ? 0 : (q > nl - 1 ? nl - 1 : q);
  const int s = (int)(((i64)(2 * q + 1) * n) / (2 * nl));
  return s < n - 1 ? s : n - 1;
}

#define LR_PX (FLT_TX + 3)
#define LR_PY (FLT_TY + 3)
#define LR_PZ (FLT_TZ + 3)

__device__ __forceinline__ float lowres_taps(const float* w, const float* p, int stride) {
  float acc = w[0] * p[0];
#pragma unroll
  for (int t = 1; t < 4; ++t) acc = acc + w[t] * p[t * stride];
  return acc;
}

template <int MC, bool VEC>
__global__ __launch_bounds__(256) void augment_lowres_kernel(const float* __restrict__ src, float* __restrict__ dst, int X,
                                                               int Y, int Z, int Mrt, int tiles_x, int tiles_y,
                                                               Seg3dLowresParams prm) {
  constexpr int MR = mc_regs<MC>;
  const int M = mc_width<MC>(Mrt);
  __shared__ float A[LR_PZ * LR_PY * LR_PX];         // the low-grid patch [nzp][nyp][nxp]; then [nzp][TY][TX] after the y pass
  __shared__ float B[LR_PZ * LR_PY * FLT_TX];        // [nzp][nyp][TX] after the x pass
  __shared__ float WX[FLT_TX][4], WY[FLT_TY][4], WZ[FLT_TZ][4];
  __shared__ int JX[FLT_TX], JY[FLT_TY], JZ[FLT_TZ], SX[LR_PX], SY[LR_PY], SZ[LR_PZ];
  int x0, y0, z0;
  filter_tile_origin(tiles_x, tiles_y, x0, y0, z0);
  const int tid = threadIdx.x;
  const int x = tid & (FLT_TX - 1), y = tid >> 5;
  const int x1 = min(x0 + FLT_TX, X) - 1, y1 = min(y0 + FLT_TY, Y) - 1, z1 = min(z0 + FLT_TZ, Z) - 1;   // last voxel of the tile
  const i64 v0 = ((i64)z0 * Y + min(y0 + y, Y - 1)) * X + min(x0 + x, X - 1);
  float out[FLT_TZ][MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) {
    if (m >= M) continue;                                                     // workgroup-uniform
    const int nx = prm.nx[m], ny = prm.ny[m], nz = prm.nz[m];
    if (nx == X && ny == Y && nz == Z) {
#pragma unroll
      for (int o = 0; o < FLT_TZ; ++o) out[o][m] = src[(v0 + (i64)min(o, z1 - z0) * Y * X) * M + m];
      continue;
    }
    const int kx = lowres_k(x0, X, nx), ky = lowres_k(y0, Y, ny), kz = lowres_k(z0, Z, nz);
    const int nxp = lowres_k(x1, X, nx) - kx + 4, nyp = lowres_k(y1, Y, ny) - ky + 4, nzp = lowres_k(z1, Z, nz) - kz + 4;
    // indices past the crop's end belong to threads that write nothing; the clamp keeps their taps inside the patch
    if (tid < FLT_TX)
      lowres_entry(min(x0 + tid, x1), X, nx, kx, WX[tid], &JX[tid]);
    else if (tid < FLT_TX + FLT_TY)
      lowres_entry(min(y0 + tid - FLT_TX, y1), Y, ny, ky, WY[tid - FLT_TX], &JY[tid - FLT_TX]);
    else if (tid < FLT_TX + FLT_TY + FLT_TZ)
      lowres_entry(min(z0 + tid - FLT_TX - FLT_TY, z1), Z, nz, kz, WZ[tid - FLT_TX - FLT_TY], &JZ[tid - FLT_TX - FLT_TY]);
    else if (tid >= 64 && tid < 64 + nxp)
      SX[tid - 64] = lowres_source(tid - 64, X, nx, kx);
    else if (tid >= 128 && tid < 128 + nyp)
      SY[tid - 128] = lowres_source(tid - 128, Y, ny, ky);
    else if (tid >= 192 && tid < 192 + nzp)
      SZ[tid - 192] = lowres_source(tid - 192, Z, nz, kz);
    __syncthreads();
    const float rx = 1.0f / (float)nxp, ry = 1.0f / (float)nyp;
    for (int e = tid; e < nzp * nyp * nxp; e += 256) {
      const int row = seg3d_fdiv(e, rx), jx = e - row * nxp;
      const int jz = seg3d_fdiv(row, ry), jy = row - jz * nyp;
      A[e] = src[(((i64)SZ[jz] * Y + SY[jy]) * X + SX[jx]) * M + m];
    }
    __syncthreads();
    for (int e = tid; e < nzp * nyp * FLT_TX; e += 256)                        // e = (jz * nyp + jy) * TX + x
      B[e] = lowres_taps(WX[e & (FLT_TX - 1)], A + (e >> 5) * nxp + JX[e & (FLT_TX - 1)], 1);
    __syncthreads();
    for (int e = tid; e < nzp * FLT_TY * FLT_TX; e += 256) {                   // e = (jz * TY + y) * TX + x
      const int ey = (e >> 5) & (FLT_TY - 1);
      A[e] = lowres_taps(WY[ey], B + ((e >> 8) * nyp + JY[ey]) * FLT_TX + (e & (FLT_TX - 1)), FLT_TX);
    }
    __syncthreads();
#pragma unroll
    for (int o = 0; o < FLT_TZ; ++o) out[o][m] = lowres_taps(WZ[o], A + JZ[o] * (FLT_TY * FLT_TX) + tid, FLT_TY * FLT_TX);
    __syncthreads();                                                           // the next modality overwrites the tables and A
  }
  if (x0 + x >= X || y0 + y >= Y) return;
#pragma unroll
  for (int o = 0; o < FLT_TZ; ++o)
    if (z0 + o < Z) mc_store_row<MC, VEC>(dst + (v0 + (i64)o * Y * X) * M, out[o], M);
}

// every modality off: dst = src, 16 bytes per thread where both bases allow it
template <bool VEC>
__global__ __launch_bounds__(256) void augment_filter_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, i64 n) {
  if constexpr (VEC) {
    const i64 n4 = n >> 2;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n4; i += (i64)gridDim.x * 256)
      reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[i];
    for (i64 i = (n4 << 2) + (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) dst[i] = src[i];
  } else {
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) dst[i] = src[i];
  }
}

static void filter_copy(const float* src, float* dst, i64 n, hipStream_t s) {
  if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0)
    hipLaunchKernelGGL(augment_filter_copy_kernel<true>, dim3(seg3d_ew_grid(n >> 2, 256)), dim3(256), 0, s, src, dst, n);
  else
    hipLaunchKernelGGL(augment_filter_copy_kernel<false>, dim3(seg3d_ew_grid(n, 256)), dim3(256), 0, s, src, dst, n);
}

// shared argument checks; n = floats of the crop
static int filter_check(const char* name, const float* src, const float* dst, int X, int Y, int Z, int M) {
  SEG3D_REQUIRE(src && dst, "%s: null buffer", name);
  SEG3D_REQUIRE(X > 0 && Y > 0 && Z > 0, "%s: crop of %d x %d x %d voxels", name, X, Y, Z);
  SEG3D_REQUIRE(M >= 1 && M <= 8, "%s: M = %d channels, 1..8 are supported", name, M);
  const i64 n = (i64)X * Y * Z * M;
  SEG3D_REQUIRE((i64)X * Y * Z <= ((i64)1 << 30), "%s: crop of %d x %d x %d voxels is too large", name, X, Y, Z);
  const uintptr_t a = (uintptr_t)src, b = (uintptr_t)dst;
  SEG3D_REQUIRE(a + (uintptr_t)n * 4 <= b || b + (uintptr_t)n * 4 <= a, "%s: src and dst overlap (the transform is out of place)",
                name);
  return SEG3D_OK;
}

template <int MC, bool VEC>
static int blur_launch(const float* src, float* dst, int X, int Y, int Z, int M, int R, const Seg3dBlurParams& prm,
                       hipStream_t s) {
  static Seg3dOncePerDevice configured;
  if (int rc = seg3d_allow_full_lds(reinterpret_cast<const void*>(&augment_blur_kernel<MC, VEC>), configured, "augment_blur"))
    return rc;
  const int ntx = seg3d_cdiv(X, FLT_TX), nty = seg3d_cdiv(Y, FLT_TY), ntz = seg3d_cdiv(Z, FLT_TZ);
  hipLaunchKernelGGL((augment_blur_kernel<MC, VEC>), dim3((unsigned)(ntx * nty * ntz), (unsigned)(M / MC)), dim3(256),
                     blur_lds_floats(MC, R) * 4, s, src, dst, X, Y, Z, M, R, ntx, nty, prm);
  return SEG3D_OK;
}

extern "C" int seg3d_augment_blur(const float* src, float* dst, int X, int Y, int Z, int M, Seg3dBlurParams params,
                                  void* stream) {
  if (int rc = filter_check("seg3d_augment_blur", src, dst, X, Y, Z, M)) return rc;
  int R = 0;
  for (int m = 0; m < M; ++m) {
    SEG3D_REQUIRE(params.radius[m] >= 0 && params.radius[m] <= 6, "seg3d_augment_blur: radius[%d] = %d, 0..6 are supported", m,
                  params.radius[m]);
    for (int k = 0; k <= params.radius[m]; ++k)
      SEG3D_REQUIRE(params.taps[m][k] >= 0.f && params.taps[m][k] <= 1.f, "seg3d_augment_blur: taps[%d][%d] = %g outside [0, 1]",
                    m, k, params.taps[m][k]);
    if (params.radius[m] > R) R = params.radius[m];
  }
  hipStream_t s = (hipStream_t)stream;
  int rc = SEG3D_OK;
  const bool vec = mc_vec_rows(M, src, dst);
  if (R == 0)
    filter_copy(src, dst, (i64)X * Y * Z * M, s);
  else if (vec && M == 4)
    rc = blur_launch<4, true>(src, dst, X, Y, Z, M, R, params, s);
  else if (vec)
    rc = blur_launch<2, true>(src, dst, X, Y, Z, M, R, params, s);
  else
    rc = blur_launch<1, false>(src, dst, X, Y, Z, M, R, params, s);
  if (rc) return rc;
  SEG3D_LAUNCH_CHECK("seg3d_augment_blur");
  return SEG3D_OK;
}

template <int MC, bool VEC>
static void lowres_launch(const float* src, float* dst, int X, int Y, int Z, int M, const Seg3dLowresParams& prm,
                          hipStream_t s) {
  const int ntx = seg3d_cdiv(X, FLT_TX), nty = seg3d_cdiv(Y, FLT_TY), ntz = seg3d_cdiv(Z, FLT_TZ);
  constexpr int KC = MC == 3 ? 0 : MC;   // there is no <3> instantiation: M = 3 runs the runtime width
  hipLaunchKernelGGL((augment_lowres_kernel<KC, VEC>), dim3((unsigned)(ntx * nty * ntz)), dim3(256), 0, s, src, dst, X, Y, Z, M,
                     ntx, nty, prm);
}

extern "C" int seg3d_augment_lowres(const float* src, float* dst, int X, int Y, int Z, int M, Seg3dLowresParams params,
                                    void* stream) {
  if (int rc = filter_check("seg3d_augment_lowres", src, dst, X, Y, Z, M)) return rc;
  SEG3D_REQUIRE(X <= (1 << 14) && Y <= (1 << 14) && Z <= (1 << 14), "seg3d_augment_lowres: axis longer than 16384 voxels");
  bool any = false;
  for (int m = 0; m < M; ++m) {
    SEG3D_REQUIRE(params.nx[m] >= 1 && params.nx[m] <= X && params.ny[m] >= 1 && params.ny[m] <= Y && params.nz[m] >= 1 &&
                      params.nz[m] <= Z,
                  "seg3d_augment_lowres: low grid %d x %d x %d of modality %d, need 1 <= n' <= n = %d x %d x %d", params.nx[m],
                  params.ny[m], params.nz[m], m, X, Y, Z);
    any = any || params.nx[m] != X || params.ny[m] != Y || params.nz[m] != Z;
  }
  hipStream_t s = (hipStream_t)stream;
  if (!any)
    filter_copy(src, dst, (i64)X * Y * Z * M, s);
  else   // only the stores are rows: the sources are gathered voxel by voxel
    MC_DISPATCH(lowres_launch, M, mc_vec_rows(M, dst), (src, dst, X, Y, Z, M, params, s));
  SEG3D_LAUNCH_CHECK("seg3d_augment_lowres");
  return SEG3D_OK;
}
