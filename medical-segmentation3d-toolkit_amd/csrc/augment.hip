// augment.hip -- intensity augmentation of a normalised training crop, in place on the device (DESIGN.md section 7 row f8;
// the reference has no augmentation beyond the random crop geometry of dataloader/dataset.py:166-200).
// The crop is channels-last [z][y][x][M] (M = 1: planar).  Per modality m, with (mn, mx, mean) of the crop's channel m:
//   1. brightness  y = x * b                                  (b > 0; the statistics scale with it)
//   2. contrast    y = clamp(mean + c * (y - mean), mn, mx)   (c > 0; monotone, so the new range [lo, hi] is the map
//                                                              applied to mn and mx -- no second statistics pass)
//   3. gamma       hi - lo >= 1e-7: r = (y - lo) / (hi - lo), r = 1 - r if invert, r = r^g, r = 1 - r if invert,
//                  y = lo + r * (hi - lo); otherwise unchanged (g > 0)
//   4. noise       y += sigma * n, n = sqrt(-2 ln u1) cos(2 pi u2), (u1, u2) = ((r0 + 1) 2^-32, r1 2^-32) from
//                  Philox4x32-10 with key (seed_lo, seed_hi) and counter (v_lo, v_hi, m, 0), v = (z * Y + y) * X + x: a
//                  function of the voxel and the modality alone, whatever the memory layout, the grid or M
// A transform with a neutral parameter (b = 1, c = 1, g = 1, sigma = 0) is skipped exactly.  min / max are exact, the mean
// comes from an fp64 sum reduced in a fixed order (partial pass -> finalize, no atomics): two runs are bit-equal.  fp32
// arithmetic, no FMA contraction (-ffp-contract=off).  HBM-bound byte movers: one read for the statistics (only with
// contrast or gamma), one read + one write for the apply pass, 16- / 8-byte rows for M = 4 / 2.
#include "mc_device.h"
#include "seg3d_hip.h"

// partial[(m * nblk + blk) * 3 + (0, 1, 2)] = (sum, min, max) of modality m over a chunk of voxels, as doubles
template <int MC, bool VEC>
__global__ __launch_bounds__(256) void augment_stats_partial_kernel(const float* __restrict__ crop,
                                                                      double* __restrict__ partial, int Mrt, i64 nv,
                                                                      int nblk) {
  constexpr int MR = mc_regs<MC>;
  const int M = mc_width<MC>(Mrt);
  __shared__ double red_s[MR][4];
  __shared__ float red_lo[MR][4], red_hi[MR][4];
  double s[MR];
  float lo[MR], hi[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) {
    s[m] = 0.0;
    lo[m] = INFINITY;
    hi[m] = -INFINITY;
  }
  mc_chunk_walk<MC, VEC>(
      nv, M, [&](i64 e) { return crop + e * M; },
      [&](const float* r) {
#pragma unroll
        for (int m = 0; m < MR; ++m) {
          s[m] += (double)r[m];
          lo[m] = fminf(lo[m], r[m]);
          hi[m] = fmaxf(hi[m], r[m]);
        }
      });
  mc_stat_park(s, red_s, 0);
#pragma unroll
  for (int m = 0; m < MR; ++m) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      lo[m] = fminf(lo[m], __shfl_down(lo[m], off, 64));
      hi[m] = fmaxf(hi[m], __shfl_down(hi[m], off, 64));
    }
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      red_lo[m][threadIdx.x >> 6] = lo[m];
      red_hi[m][threadIdx.x >> 6] = hi[m];
    }
  }
  __syncthreads();
  if (threadIdx.x < M) {
    const int m = threadIdx.x;
    double* out = partial + ((i64)m * nblk + blockIdx.x) * 3;
    out[0] = mc_stat_total(red_s[m]);
    out[1] = (double)fminf(fminf(red_lo[m][0], red_lo[m][1]), fminf(red_lo[m][2], red_lo[m][3]));
    out[2] = (double)fmaxf(fmaxf(red_hi[m][0], red_hi[m][1]), fmaxf(red_hi[m][2], red_hi[m][3]));
  }
}

// stats[m] = (mn, mx, mean) as float32; one workgroup of 64 threads per modality, fixed order
__global__ __launch_bounds__(64) void augment_stats_finalize_kernel(const double* __restrict__ partial,
                                                                      float* __restrict__ stats, int nblk, double nv) {
  const int m = blockIdx.x;
  double s = 0.0, lo = INFINITY, hi = -INFINITY;
  for (int k = threadIdx.x; k < nblk; k += 64) {
    const double* p = partial + ((i64)m * nblk + k) * 3;
    s += p[0];
    lo = fmin(lo, p[1]);
    hi = fmax(hi, p[2]);
  }
  s = wave_sum_d(s);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = fmin(lo, __shfl_down(lo, off, 64));
    hi = fmax(hi, __shfl_down(hi, off, 64));
  }
  if (threadIdx.x == 0) {
    stats[3 * m + 0] = (float)lo;
    stats[3 * m + 1] = (float)hi;
    stats[3 * m + 2] = (float)(s / nv);
  }
}

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): plain integer multiplies and xors
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned& r0, unsigned& r1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1,
                   n3 = (unsigned)p0;
    c0 = n0;
    c1 = n1;
    c2 = n2;
    c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  r0 = c0;
  r1 = c1;
}

__device__ __forceinline__ float augment_normal(i64 v, int m, unsigned seed_lo, unsigned seed_hi) {
  unsigned r0, r1;
  philox4x32_10((unsigned)v, (unsigned)((unsigned long long)v >> 32), (unsigned)m, 0u, seed_lo, seed_hi, r0, r1);
  const float u1 = ((float)r0 + 1.0f) * 2.3283064365386963e-10f;   // (r0 + 1) 2^-32 in (0, 1]
  const float u2 = (float)r1 * 2.3283064365386963e-10f;
  return sqrtf(-2.0f * logf(u1)) * cosf(6.2831853071795865f * u2);
}

// one modality's value: the four steps of the header comment; st = (mn, mx, mean) of the channel (unused without contrast
// and gamma: the launcher then passes no statistics)
__device__ __forceinline__ float augment_value(float x, const Seg3dIntensity& p, float mn, float mx, float mean, i64 v, int m,
                                               unsigned seed_lo, unsigned seed_hi) {
  float y = x;
  if (p.brightness != 1.0f) {
    y = y * p.brightness;
    mn = mn * p.brightness;
    mx = mx * p.brightness;
    mean = mean * p.brightness;
  }
  float lo = mn, hi = mx;
  if (p.contrast != 1.0f) {
    y = fminf(fmaxf(mean + p.contrast * (y - mean), mn), mx);
    lo = fminf(fmaxf(mean + p.contrast * (mn - mean), mn), mx);
    hi = fminf(fmaxf(mean + p.contrast * (mx - mean), mn), mx);
  }
  if (p.gamma != 1.0f && hi - lo >= 1e-7f) {
    const float range = hi - lo;
    float r = fminf(fmaxf((y - lo) / range, 0.0f), 1.0f);
    if (p.invert) r = 1.0f - r;
    r = powf(r, p.gamma);
    if (p.invert) r = 1.0f - r;
    y = lo + r * range;
  }
  if (p.sigma != 0.0f) y = y + p.sigma * augment_normal(v, m, seed_lo, seed_hi);
  return y;
}

template <int MC, bool VEC>
__global__ __launch_bounds__(256) void augment_apply_kernel(float* crop, const float* __restrict__ stats, int Mrt, i64 nv,
                                                              Seg3dIntensityParams prm) {
  constexpr int MR = mc_regs<MC>;
  const int M = mc_width<MC>(Mrt);
  float mn[MR], mx[MR], mean[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) {
    const bool have = stats && m < M;
    mn[m] = have ? stats[3 * m + 0] : 0.f;
    mx[m] = have ? stats[3 * m + 1] : 0.f;
    mean[m] = have ? stats[3 * m + 2] : 0.f;
  }
  for (i64 v = (i64)blockIdx.x * 256 + threadIdx.x; v < nv; v += (i64)gridDim.x * 256) {
    float* row = crop + v * M;
    if constexpr (MC > 0) {
      float r[MC];
      mc_load_row<MC, VEC>(row, r);
#pragma unroll
      for (int m = 0; m < MC; ++m) r[m] = augment_value(r[m], prm.m[m], mn[m], mx[m], mean[m], v, m, prm.seed_lo, prm.seed_hi);
      mc_store_row<MC, VEC>(row, r);
    } else {   // the runtime width goes channel by channel, in place: held as a row the eight values cost 8 more registers
#pragma unroll
      for (int m = 0; m < MR; ++m)
        if (m < M) row[m] = augment_value(row[m], prm.m[m], mn[m], mx[m], mean[m], v, m, prm.seed_lo, prm.seed_hi);
    }
  }
}

static long long augment_stat_blocks(long long nv) { return (nv + MC_STAT_CHUNK - 1) / MC_STAT_CHUNK; }

// doubles of workspace for seg3d_augment_intensity: M * blocks * 3 partials + the M * 3 float32 statistics behind them
extern "C" long long seg3d_augment_intensity_workspace_doubles(int X, int Y, int Z, int M) {
  if (X <= 0 || Y <= 0 || Z <= 0 || M <= 0) return 0;
  return (long long)M * augment_stat_blocks((long long)X * Y * Z) * 3 + 2 * (long long)M;
}

template <int MC, bool VEC>
static void augment_launch(float* crop, double* partial, float* stats, int M, i64 nv, int nblk, bool need_stats,
                           const Seg3dIntensityParams& prm, int apply_grid, hipStream_t s) {
  if (need_stats) {
    hipLaunchKernelGGL((augment_stats_partial_kernel<MC, VEC>), dim3(nblk), dim3(256), 0, s, crop, partial, M, nv, nblk);
    hipLaunchKernelGGL(augment_stats_finalize_kernel, dim3(M), dim3(64), 0, s, partial, stats, nblk, (double)nv);
  }
  hipLaunchKernelGGL((augment_apply_kernel<MC, VEC>), dim3(apply_grid), dim3(256), 0, s, crop, need_stats ? stats : nullptr, M,
                     nv, prm);
}

// crop [Z][Y][X][M] float32, in place.  workspace: seg3d_augment_intensity_workspace_doubles doubles (may be null when no
// modality has contrast or gamma on).  grid_blocks: workgroups of the apply pass, 0 = the library's choice (the result does
// not depend on it).  Nothing is launched when every parameter is neutral.
extern "C" int seg3d_augment_intensity(float* crop, double* workspace, int X, int Y, int Z, int M,
                                       Seg3dIntensityParams params, int grid_blocks, void* stream) {
  SEG3D_REQUIRE(crop && X > 0 && Y > 0 && Z > 0, "seg3d_augment_intensity: bad arguments");
  SEG3D_REQUIRE(M >= 1 && M <= 8, "seg3d_augment_intensity: M = %d channels, 1..8 are supported", M);
  SEG3D_REQUIRE(grid_blocks >= 0 && grid_blocks <= 65536, "seg3d_augment_intensity: grid of %d workgroups", grid_blocks);
  bool any = false, need_stats = false;
  for (int m = 0; m < M; ++m) {
    const Seg3dIntensity& p = params.m[m];
    SEG3D_REQUIRE(p.brightness > 0.f && p.brightness < INFINITY, "seg3d_augment_intensity: brightness[%d] = %g must be positive", m, p.brightness);
    SEG3D_REQUIRE(p.contrast > 0.f && p.contrast < INFINITY, "seg3d_augment_intensity: contrast[%d] = %g must be positive", m, p.contrast);
    SEG3D_REQUIRE(p.gamma > 0.f && p.gamma < INFINITY, "seg3d_augment_intensity: gamma[%d] = %g must be positive", m, p.gamma);
    SEG3D_REQUIRE(p.sigma >= 0.f && p.sigma < INFINITY, "seg3d_augment_intensity: sigma[%d] = %g must be >= 0", m, p.sigma);
    const bool stats_m = p.contrast != 1.f || p.gamma != 1.f;
    need_stats = need_stats || stats_m;
    any = any || stats_m || p.brightness != 1.f || p.sigma != 0.f;
  }
  if (!any) return SEG3D_OK;
  SEG3D_REQUIRE(!need_stats || workspace, "seg3d_augment_intensity: contrast / gamma need the workspace");
  const i64 nv = (i64)X * Y * Z;
  const int nblk = (int)augment_stat_blocks(nv);
  float* stats = need_stats ? reinterpret_cast<float*>(workspace + (i64)M * nblk * 3) : nullptr;
  const int grid = grid_blocks > 0 ? grid_blocks : seg3d_ew_grid(nv, 256);
  hipStream_t s = (hipStream_t)stream;
  MC_DISPATCH(augment_launch, M, mc_vec_rows(M, crop), (crop, workspace, stats, M, nv, nblk, need_stats, params, grid, s));
  SEG3D_LAUNCH_CHECK("seg3d_augment_intensity");
  return SEG3D_OK;
}
