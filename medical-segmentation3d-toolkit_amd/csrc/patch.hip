// patch.hip -- on-device sliding-window batcher: crop + normalise patches out of a resident volume, accumulate
// the per-patch probability maps back with overlap counts, then average and arg-max.
//
// Reference path restated (file:line relative to /root/reference/segmentation3d):
//   * ROI slice + crop_normalizers[0] on the ROI                     core/seg_infer.py:221-224
//       AdaptiveNormalizer: (x - mean(ROI)) / max(std(ROI), 1e-6), clip to +-clip_sigma   utils/normalizer.py:55-62
//       FixedNormalizer:    (x - mean) / stddev, optional clip to [-1, 1]                 utils/normalizer.py:22-25,
//                                                                                          utils/image_tools.py:221-238
//   * acc[c][z0:z1, y0:y1, x0:x1] += prob_c ; count[...] += 1.0       utils/image_tools.py:435-469, seg_infer.py:313-322
//   * probs *= 1 / count ; mask = argmax_c -> int8                    core/seg_infer.py:325-327, 336-339
// Voxel (x, y, z) of a volume with size (X, Y, Z) lives at [z][y][x] (utils/image_tools.py:448,465).
// All kernels are HBM-bound byte movers over fp32 / int8 data.
#include "seg3d_imagegrid.h"
#include "mc_device.h"
#include "seg3d_hip.h"

// SEG3D_LAUNCH_CHECK for a launch chain entered under several names: "<entry><stage>: kernel launch failed: ..."
#define PATCH_LAUNCH_CHECK(name, stage)                                                           \
  do {                                                                                            \
    hipError_t e__ = hipGetLastError();                                                           \
    if (e__ != hipSuccess) {                                                                      \
      seg3d_set_error("%s%s: kernel launch failed: %s", name, stage, hipGetErrorString(e__));     \
      return SEG3D_ERR_LAUNCH;                                                                    \
    }                                                                                             \
  } while (0)

// mean_std[row] = (mean, max(population std, 1e-6)) as float32, one row of nblk partials per (patch, modality)
__global__ __launch_bounds__(64) void patch_stats_finalize_kernel(const double* __restrict__ partial,
                                                                    float* __restrict__ mean_std, int nblk, double nv) {
  const int p = blockIdx.x;
  double s = 0.0, ss = 0.0;
  for (int k = threadIdx.x; k < nblk; k += 64) {
    s += partial[((i64)p * nblk + k) * 2];
    ss += partial[((i64)p * nblk + k) * 2 + 1];
  }
  s = wave_sum_d(s);
  ss = wave_sum_d(ss);
  if (threadIdx.x == 0) {
    const double mean = s / nv;
    double var = ss / nv - mean * mean;
    if (var < 0.0) var = 0.0;
    float sd = (float)sqrt(var);
    if (sd < 1e-6f) sd = 1e-6f;
    mean_std[2 * p] = (float)mean;
    mean_std[2 * p + 1] = sd;
  }
}

extern "C" long long seg3d_patch_stats_blocks(int bx, int by, int bz) {
  return ((long long)bx * by * bz + MC_STAT_CHUNK - 1) / MC_STAT_CHUNK;
}

// ---- gather: M co-registered modalities in one launch chain (dataset.py:199-203 crops and normalises a list of images
// with crop_normalizers[idx]; core/seg_infer.py:221-224 applies crop_normalizers[0] to the single one).  The volume is
// channels-last [Z][Y][X][M]; the batch is [P][bz][by][bx][M] (NDHWC).  ONE stats pass reads each patch once for all
// modalities; the chunking, the fp64 summation order, the finalisation and the float expression of the normalisation are
// per (patch, modality) and do not depend on M, so channel m of an M-modality gather is bit-identical to the M = 1 gather
// of plane m with normaliser m.  A single-modality volume [Z][Y][X] is the M = 1 case of the same memory, and so is its
// batch [P][1][bz][by][bx]: seg3d_patch_gather_normalize(_flip) are the M = 1 entries.
// <MC, VEC>: the row width of the instantiation, mc_device.h.

// partial[(p * M + m)][blk][2] = (sum, sum of squares) in fp64 of modality m over a chunk of patch p's voxels
template <int MC, bool VEC>
__global__ __launch_bounds__(256) void patch_stats_partial_mc_kernel(const float* __restrict__ vol,
                                                                       const int* __restrict__ starts,
                                                                       double* __restrict__ partial, int Mrt, int Y, int X,
                                                                       int bx, int by, int bz, int nblk) {
  constexpr int MR = mc_regs<MC>;
  const int M = mc_width<MC>(Mrt);
  __shared__ double red[MR][8];
  const int p = blockIdx.y;
  const int sx = starts[3 * p], sy = starts[3 * p + 1], sz = starts[3 * p + 2];
  double s[MR], ss[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) s[m] = ss[m] = 0.0;
  mc_chunk_walk<MC, VEC>(
      (i64)bx * by * bz, M,
      [&](i64 e) {
        const int lx = (int)(e % bx);
        const i64 t = e / bx;
        const int ly = (int)(t % by), lz = (int)(t / by);
        return vol + (((i64)(sz + lz) * Y + (sy + ly)) * X + (sx + lx)) * M;
      },
      [&](const float* r) {
#pragma unroll
        for (int m = 0; m < MR; ++m) {
          const double v = (double)r[m];
          s[m] += v;
          ss[m] += v * v;
        }
      });
  mc_stat_park(s, red, 0);
  mc_stat_park(ss, red, 4);
  __syncthreads();
  if (threadIdx.x < M) {
    const int m = threadIdx.x;
    const i64 row = ((i64)p * M + m) * nblk + blockIdx.x;
    partial[row * 2 + 0] = mc_stat_total(red[m]);
    partial[row * 2 + 1] = mc_stat_total(red[m] + 4);
  }
}

// batch[p][lz][ly][lx][m] = clip_m((vol[...][m] - mean_pm) / std_pm)
template <int MC, bool VEC, bool FLIP>
// (vol and batch may be the same buffer: a crop normalised in place, P = 1 and the box = the volume; never with FLIP)
// FLIP: the row of M channels is read at the local position mirrored along the axes of `flip` (bit 0 = x, 1 = y, 2 = z);
// channels are innermost, so a mirrored row is still one 8- / 16-byte load
__global__ __launch_bounds__(256) void patch_gather_normalize_mc_kernel(const float* vol, const int* __restrict__ starts,
                                                                          const float* __restrict__ mean_std, float* batch, int Mrt, int Y, int X,
                                                                          int bx, int by, int bz, int P,
                                                                          Seg3dNormalizers nrm, int flip) {
  constexpr int MR = mc_regs<MC>;
  const int M = mc_width<MC>(Mrt);
  const i64 nv = (i64)bx * by * bz;
  const i64 total = nv * P;
  for (i64 idx = (i64)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (i64)gridDim.x * 256) {
    const int p = (int)(idx / nv);
    const i64 e = idx - (i64)p * nv;
    int lx = (int)(e % bx);
    const i64 t = e / bx;
    int ly = (int)(t % by), lz = (int)(t / by);
    if constexpr (FLIP) {
      if (flip & 1) lx = bx - 1 - lx;
      if (flip & 2) ly = by - 1 - ly;
      if (flip & 4) lz = bz - 1 - lz;
    }
    const int sx = starts[3 * p], sy = starts[3 * p + 1], sz = starts[3 * p + 2];
    const float* row = vol + (((i64)(sz + lz) * Y + (sy + ly)) * X + (sx + lx)) * M;
    float r[MR];
    mc_load_row<MC, VEC>(row, r, M, 0.f);
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      const Seg3dNormalizer& n = nrm.n[m];
      const bool adaptive = n.type == 1;
      const float mean = adaptive ? mean_std[((i64)p * M + m) * 2] : n.mean;
      const float sd = adaptive ? mean_std[((i64)p * M + m) * 2 + 1] : n.stddev;
      float v = (r[m] - mean) / sd;
      if (n.clip) {
        if (v < n.clip_lo) v = n.clip_lo;
        if (v > n.clip_hi) v = n.clip_hi;
      }
      r[m] = v;
    }
    mc_store_row<MC, VEC>(batch + idx * M, r, M);
  }
}

extern "C" long long seg3d_patch_stats_mc_doubles(int bx, int by, int bz, int P, int M) {
  return (long long)P * M * seg3d_patch_stats_blocks(bx, by, bz) * 2;
}

template <int MC, bool VEC>
static int patch_gather_normalize_mc_launch(const char* name, const float* volume, const int* starts, float* batch,
                                            double* workspace, float* mean_std, int M, int Y, int X, int bx, int by, int bz,
                                            int P, const Seg3dNormalizers& nrm, bool any_adaptive, int flip,
                                            hipStream_t s) {
  if (any_adaptive) {
    const int nblk = (int)seg3d_patch_stats_blocks(bx, by, bz);
    hipLaunchKernelGGL((patch_stats_partial_mc_kernel<MC, VEC>), dim3(nblk, P), dim3(256), 0, s, volume, starts, workspace,
                       M, Y, X, bx, by, bz, nblk);
    PATCH_LAUNCH_CHECK(name, "(stats)");
    hipLaunchKernelGGL(patch_stats_finalize_kernel, dim3(P * M), dim3(64), 0, s, workspace, mean_std, nblk,
                       (double)bx * by * bz);
    PATCH_LAUNCH_CHECK(name, "(finalize)");
  }
  const i64 total = (i64)bx * by * bz * P;
  if (flip)
    hipLaunchKernelGGL((patch_gather_normalize_mc_kernel<MC, VEC, true>), dim3(seg3d_ew_grid(total, 256)), dim3(256), 0, s,
                       volume, starts, mean_std, batch, M, Y, X, bx, by, bz, P, nrm, flip);
  else
    hipLaunchKernelGGL((patch_gather_normalize_mc_kernel<MC, VEC, false>), dim3(seg3d_ew_grid(total, 256)), dim3(256), 0, s,
                       volume, starts, mean_std, batch, M, Y, X, bx, by, bz, P, nrm, 0);
  PATCH_LAUNCH_CHECK(name, "");
  return SEG3D_OK;
}

// volume [Z][Y][X][M], batch [P][bz][by][bx][M]; starts: device int32 [P][3] as (x, y, z) (the sliding window's control
// block).  norms.n[m] for m < M: type 0 = fixed (mean, stddev, clip to [clip_lo, clip_hi] when clip != 0), 1 = adaptive
// (the patch's own mean / std, clip to [clip_lo, clip_hi]), -1 = none.  workspace: seg3d_patch_stats_mc_doubles doubles,
// mean_std: P * M * 2 floats (both used only when a modality is adaptive).  batch may be volume itself when P = 1, the
// start is 0 and the box is the whole volume (a training crop normalised in place), but never for a mirrored gather.
// flip: mirror mask of the gathered patches (bit 0 = x, 1 = y, 2 = z; 0 = the plain gather).  The statistics of the
// adaptive normaliser are taken over the same voxels in the same order whatever the mask, so mean / std are those of the
// un-mirrored patch bit for bit and a mirrored gather equals the flipped plain gather exactly.
// name: the entry the caller used, for the messages.
static int patch_gather_normalize_mc_impl(const char* name, const float* volume, const int* starts, float* batch,
                                          double* workspace, float* mean_std, int Z, int Y, int X, int bx, int by, int bz,
                                          int P, int M, const Seg3dNormalizers& norms, int flip, void* stream) {
  SEG3D_REQUIRE(flip >= 0 && flip <= 7, "%s: flip mask %d outside 0..7", name, flip);
  SEG3D_REQUIRE(volume && starts && batch && P > 0, "%s: bad arguments", name);
  SEG3D_REQUIRE(M >= 1 && M <= 8, "%s: M = %d modalities, 1..8 are supported", name, M);
  SEG3D_REQUIRE(bx > 0 && by > 0 && bz > 0 && bx <= X && by <= Y && bz <= Z,
                "%s: box (%d,%d,%d) does not fit volume (%d,%d,%d)", name, bx, by, bz, X, Y, Z);
  SEG3D_REQUIRE(flip == 0 || volume != batch, "%s: a mirrored gather cannot run in place", name);
  Seg3dNormalizers nrm = {};
  bool any_adaptive = false;
  for (int m = 0; m < 8; ++m) {
    Seg3dNormalizer n = {-1, 0.f, 1.f, 0, -1.f, 1.f};
    if (m < M) {
      n = norms.n[m];
      if (n.type == 1) {
        SEG3D_REQUIRE(n.clip_hi > n.clip_lo, "%s: modality %d: empty clip range", name, m);
        n.mean = 0.f;
        n.stddev = 1.f;
        n.clip = 1;
        any_adaptive = true;
      } else if (n.type == 0) {
        SEG3D_REQUIRE(n.stddev > 0.f, "%s: modality %d: stddev must be positive", name, m);
        n.clip = n.clip ? 1 : 0;
      } else if (n.type == -1) {
        n = Seg3dNormalizer{-1, 0.f, 1.f, 0, -1.f, 1.f};
      } else {
        SEG3D_UNSUPPORTED("%s: modality %d: unsupported normalization type %d", name, m, n.type);
      }
    }
    nrm.n[m] = n;
  }
  SEG3D_REQUIRE(!any_adaptive || (workspace && mean_std), "%s: adaptive normaliser needs workspace and mean_std", name);
  hipStream_t s = (hipStream_t)stream;
  MC_DISPATCH(return patch_gather_normalize_mc_launch, M, mc_vec_rows(M, volume, batch),
              (name, volume, starts, batch, workspace, mean_std, M, Y, X, bx, by, bz, P, nrm, any_adaptive, flip, s));
}

extern "C" int seg3d_patch_gather_normalize_mc(const float* volume, const int* starts, float* batch, double* workspace,
                                               float* mean_std, int Z, int Y, int X, int bx, int by, int bz, int P, int M,
                                               Seg3dNormalizers norms, void* stream) {
  return patch_gather_normalize_mc_impl("seg3d_patch_gather_normalize_mc", volume, starts, batch, workspace, mean_std, Z, Y,
                                        X, bx, by, bz, P, M, norms, 0, stream);
}

// the multi-modality gather with every patch mirrored by flip_mask (0..7): batch[p][lz][ly][lx][m] is the normalised
// voxel at start_p + (fx ? bx-1-lx : lx, fy ? by-1-ly : ly, fz ? bz-1-lz : lz), i.e. torch.flip of the plain gather;
// batch must not alias volume unless flip_mask is 0
extern "C" int seg3d_patch_gather_normalize_mc_flip(const float* volume, const int* starts, float* batch, double* workspace,
                                                    float* mean_std, int Z, int Y, int X, int bx, int by, int bz, int P,
                                                    int M, Seg3dNormalizers norms, int flip_mask, void* stream) {
  return patch_gather_normalize_mc_impl("seg3d_patch_gather_normalize_mc_flip", volume, starts, batch, workspace, mean_std,
                                        Z, Y, X, bx, by, bz, P, M, norms, flip_mask, stream);
}

// The single-modality entries are the M = 1 case: volume [Z][Y][X], batch [P][1][bz][by][bx], workspace
// P * seg3d_patch_stats_blocks * 2 doubles and mean_std P * 2 floats (adaptive only) -- the M = 1 layouts.
// normalizer_type: 0 = fixed (mean, stddev, clip to [-1,1] when clip != 0), 1 = adaptive (clip to +-clip_sigma), -1 = none.
static int patch_gather_normalize_single(const char* name, const float* volume, const int* starts, float* batch,
                                         double* workspace, float* mean_std, int Z, int Y, int X, int bx, int by, int bz,
                                         int P, int normalizer_type, float mean, float stddev, int clip, float clip_sigma,
                                         int flip, void* stream) {
  Seg3dNormalizers norms = {};
  if (normalizer_type == 1) {
    SEG3D_REQUIRE(clip_sigma > 0.f, "%s: clip_sigma must be positive", name);
    norms.n[0] = Seg3dNormalizer{1, 0.f, 1.f, 1, -clip_sigma, clip_sigma};
  } else if (normalizer_type == 0) {
    SEG3D_REQUIRE(stddev > 0.f, "%s: stddev must be positive", name);
    norms.n[0] = Seg3dNormalizer{0, mean, stddev, clip, -1.f, 1.f};
  } else if (normalizer_type == -1) {
    norms.n[0] = Seg3dNormalizer{-1, 0.f, 1.f, 0, -1.f, 1.f};
  } else {
    SEG3D_UNSUPPORTED("%s: unsupported normalization type %d", name, normalizer_type);
  }
  return patch_gather_normalize_mc_impl(name, volume, starts, batch, workspace, mean_std, Z, Y, X, bx, by, bz, P, 1, norms,
                                        flip, stream);
}

extern "C" int seg3d_patch_gather_normalize(const float* volume, const int* starts, float* batch, double* workspace,
                                            float* mean_std, int Z, int Y, int X, int bx, int by, int bz, int P,
                                            int normalizer_type, float mean, float stddev, int clip, float clip_sigma,
                                            void* stream) {
  return patch_gather_normalize_single("seg3d_patch_gather_normalize", volume, starts, batch, workspace, mean_std, Z, Y, X,
                                       bx, by, bz, P, normalizer_type, mean, stddev, clip, clip_sigma, 0, stream);
}

// the same gather with every patch mirrored by flip_mask (0..7), see seg3d_patch_gather_normalize_mc_flip
extern "C" int seg3d_patch_gather_normalize_flip(const float* volume, const int* starts, float* batch, double* workspace,
                                                 float* mean_std, int Z, int Y, int X, int bx, int by, int bz, int P,
                                                 int normalizer_type, float mean, float stddev, int clip, float clip_sigma,
                                                 int flip_mask, void* stream) {
  return patch_gather_normalize_single("seg3d_patch_gather_normalize_flip", volume, starts, batch, workspace, mean_std, Z, Y,
                                       X, bx, by, bz, P, normalizer_type, mean, stddev, clip, clip_sigma, flip_mask, stream);
}

// ---- scatter.  One thread per volume voxel of the batch's bounding box; patches are applied in list order so the float
// summation order per voxel equals the reference's sequential loop (no atomics, reproducible).  The bounding box and the
// number of valid patches come from a small DEVICE control block so that a captured hipGraph can be replayed for every
// batch with unchanged kernel arguments:  ctl = {lo_x, lo_y, lo_z, extent_x, extent_y, extent_z, n_valid}.
// Weighted and / or mirrored accumulation:
//   w = (g_z[lz] * g_y[ly]) * g_x[lx]   (wtab = x table, y table, z table: bx + by + bz floats; WEIGHTED = false: w = 1)
//   acc[c][v] = acc[c][v] + (w * prob),  count[v] = count[v] + w     -- a rounded multiply, then a rounded add
// (the file is built with -ffp-contract=off and the pragma below pins it, so no FMA is formed and the result is bit-equal
// to a float32 loop on the host; with w = 1 the product is the probability itself and the count grows by 1.0f per patch,
// the reference's plain accumulation).  The probabilities of a patch are stored mirrored by `flip`: the value that belongs
// to local voxel (lx, ly, lz) is read at the mirrored position (FLIP = false: flip is 0, no mirror code is compiled); the
// tables are symmetric, so the weight needs no mirror, but it is indexed with the un-mirrored position all the same.  A
// mirror along x reverses the lanes' addresses inside one contiguous row.  The table reads are L1 / L2 hits (a few
// hundred bytes shared by every thread).
template <bool WEIGHTED, bool FLIP>
__global__ __launch_bounds__(256) void patch_scatter_blend_kernel(const float* __restrict__ probs,
                                                                    const int* __restrict__ starts,
                                                                    const int* __restrict__ ctl,
                                                                    const float* __restrict__ wtab, float* __restrict__ acc,
                                                                    float* __restrict__ count, int Z, int Y, int X, int bx,
                                                                    int by, int bz, int C, int flip) {
#pragma clang fp contract(off)
  const int lox = ctl[0], loy = ctl[1], loz = ctl[2], ex = ctl[3], ey = ctl[4], ez = ctl[5], P = ctl[6];
  const i64 total = (i64)ex * ey * ez;
  const i64 vol = (i64)Z * Y * X;
  const i64 nv = (i64)bx * by * bz;
  for (i64 idx = (i64)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (i64)gridDim.x * 256) {
    const int x = lox + (int)(idx % ex);
    const i64 t = idx / ex;
    const int y = loy + (int)(t % ey), z = loz + (int)(t / ey);
    if (x >= X || y >= Y || z >= Z) continue;
    const i64 v = ((i64)z * Y + y) * X + x;
    float cnt = count[v];
    bool hit = false;
    for (int p = 0; p < P; ++p) {
      const int lx = x - starts[3 * p], ly = y - starts[3 * p + 1], lz = z - starts[3 * p + 2];
      if (lx >= 0 && lx < bx && ly >= 0 && ly < by && lz >= 0 && lz < bz) {
        float w = 1.0f;
        if constexpr (WEIGHTED) w = (wtab[bx + by + lz] * wtab[bx + ly]) * wtab[lx];
        int mx = lx, my = ly, mz = lz;
        if constexpr (FLIP) {
          if (flip & 1) mx = bx - 1 - lx;
          if (flip & 2) my = by - 1 - ly;
          if (flip & 4) mz = bz - 1 - lz;
        }
        const i64 e = ((i64)mz * by + my) * bx + mx;
        for (int c = 0; c < C; ++c) {
          const float wp = w * probs[((i64)p * C + c) * nv + e];
          acc[(i64)c * vol + v] = acc[(i64)c * vol + v] + wp;
        }
        cnt = cnt + w;
        hit = true;
      }
    }
    if (hit) count[v] = cnt;
  }
}

// probs [P][C][bz][by][bx] -> acc [C][Z][Y][X] += w * prob, count [Z][Y][X] += w.  starts_xyz: device int32 [P][3];
// ctl: device int32 [7] (see kernel); max_box_voxels: host upper bound of the bounding-box volume (sizes the grid).
// wtab: device, bx + by + bz floats (x table, y table, z table), NULL = constant weight 1; flip (0..7): probs of every patch
// are stored mirrored by it.
static int patch_scatter(const char* name, const float* probs, const int* starts, const int* ctl, const float* wtab,
                         float* acc, float* count, int Z, int Y, int X, int bx, int by, int bz, int C, int flip,
                         long long max_box_voxels, void* stream) {
  SEG3D_REQUIRE(flip >= 0 && flip <= 7, "%s: flip mask %d outside 0..7", name, flip);
  SEG3D_REQUIRE(probs && starts && ctl && acc && count && C > 0, "%s: bad arguments", name);
  SEG3D_REQUIRE(bx > 0 && by > 0 && bz > 0 && bx <= X && by <= Y && bz <= Z && max_box_voxels > 0, "%s: bad box", name);
  auto kernel = wtab ? (flip ? patch_scatter_blend_kernel<true, true> : patch_scatter_blend_kernel<true, false>)
                     : (flip ? patch_scatter_blend_kernel<false, true> : patch_scatter_blend_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(seg3d_ew_grid(max_box_voxels, 256)), dim3(256), 0, (hipStream_t)stream, probs, starts, ctl,
                     wtab, acc, count, Z, Y, X, bx, by, bz, C, flip);
  SEG3D_LAUNCH_CHECK(name);
  return SEG3D_OK;
}

// the reference's accumulation: every patch counts 1, nothing is mirrored -- seg3d_patch_scatter_blend with wtab = NULL and
// flip_mask = 0
extern "C" int seg3d_patch_scatter_accumulate(const float* probs, const int* starts, const int* ctl, float* acc,
                                              float* count, int Z, int Y, int X, int bx, int by, int bz, int C,
                                              long long max_box_voxels, void* stream) {
  return patch_scatter("seg3d_patch_scatter_accumulate", probs, starts, ctl, nullptr, acc, count, Z, Y, X, bx, by, bz, C, 0,
                       max_box_voxels, stream);
}

// Gaussian importance weights and / or mirrored inputs
extern "C" int seg3d_patch_scatter_blend(const float* probs, const int* starts, const int* ctl, const float* wtab,
                                         float* acc, float* count, int Z, int Y, int X, int bx, int by, int bz, int C,
                                         int flip_mask, long long max_box_voxels, void* stream) {
  return patch_scatter("seg3d_patch_scatter_blend", probs, starts, ctl, wtab, acc, count, Z, Y, X, bx, by, bz, C, flip_mask,
                       max_box_voxels, stream);
}

// acc[c][v] *= 1/count[v] (in place);  mask[v] = argmax_c (first maximum: label_first_max, seg3d_imagegrid.h), int8.
// A voxel no patch covered (count 0: bounding-box runs of the coarse -> fine cascade) gets probabilities 0 and class 0: the
// reference divides SimpleITK images (core/seg_infer.py:325-327), and ITK's Div functor yields NumericTraits::max() -- not
// inf -- for a zero denominator, so its product with the zero accumulator is 0, never NaN.
__global__ __launch_bounds__(256) void finalize_argmax_kernel(float* __restrict__ acc, const float* __restrict__ count,
                                                                signed char* __restrict__ mask, int C, i64 vol,
                                                                i64 cstride) {
  for (i64 v = (i64)blockIdx.x * 256 + threadIdx.x; v < vol; v += (i64)gridDim.x * 256) {
    const float cnt = count[v];
    const float r = cnt > 0.f ? 1.0f / cnt : 0.f;
    int best = 0;
    float bv = 0.f;
    for (int c = 0; c < C; ++c) {
      const float p = acc[(i64)c * cstride + v] * r;
      acc[(i64)c * cstride + v] = p;
      label_first_max(c, p, best, bv);
    }
    if (mask) mask[v] = (signed char)best;
  }
}

// class_stride: elements between the class planes of acc (the whole volume; `voxels` may be a z-slab of it -- a rank of
// the sharded sliding window finalizes only the slab it owns); 0 = voxels
extern "C" int seg3d_finalize_argmax(float* acc, const float* count, signed char* mask, int C, long long voxels,
                                     long long class_stride, void* stream) {
  SEG3D_REQUIRE(acc && count && C > 0 && voxels > 0 && (class_stride == 0 || class_stride >= voxels),
                "seg3d_finalize_argmax: bad arguments");
  hipLaunchKernelGGL(finalize_argmax_kernel, dim3(seg3d_ew_grid(voxels, 256)), dim3(256), 0, (hipStream_t)stream, acc, count,
                     mask, C, (i64)voxels, (i64)(class_stride ? class_stride : voxels));
  SEG3D_LAUNCH_CHECK("seg3d_finalize_argmax");
  return SEG3D_OK;
}

// Region-based inference: acc[r][v] *= 1/count[v] (in place), then the sequential overwrite
// rule (label_region_overwrite, seg3d_imagegrid.h) -- mask = 0; for r = 0 .. R-1 in order: p_r > 0.5 (strictly) sets mask =
// order[r] -- so regions are listed from the
// largest to the smallest.  count 0: probabilities 0 and mask 0, as in finalize_argmax_kernel.
// (a byte array, not RegionOrder's two words: unrolled, those put all 16 labels in SGPRs -- 104, 7 waves, 11 % slower at R = 16)
struct RegionOrderBytes {
  signed char v[16];
};

__global__ __launch_bounds__(256) void finalize_regions_kernel(float* __restrict__ acc, const float* __restrict__ count,
                                                                 signed char* __restrict__ mask, int R, RegionOrderBytes order,
                                                                 i64 vol, i64 cstride) {
  for (i64 v = (i64)blockIdx.x * 256 + threadIdx.x; v < vol; v += (i64)gridDim.x * 256) {
    const float cnt = count[v];
    const float rc = cnt > 0.f ? 1.0f / cnt : 0.f;
    int m = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (r < R) {
        const float p = acc[(i64)r * cstride + v] * rc;
        acc[(i64)r * cstride + v] = p;
        m = label_region_overwrite(p, order.v[r], m);
      }
    if (mask) mask[v] = (signed char)m;
  }
}

// order_host: R host ints in 1..127 (the mask is int8); class_stride as in seg3d_finalize_argmax
extern "C" int seg3d_finalize_regions(float* acc, const float* count, signed char* mask, int R, const int* order_host,
                                      long long voxels, long long class_stride, void* stream) {
  SEG3D_REQUIRE(acc && count && order_host && voxels > 0 && (class_stride == 0 || class_stride >= voxels),
                "seg3d_finalize_regions: bad arguments");
  SEG3D_REQUIRE(R >= 1 && R <= 16, "seg3d_finalize_regions: %d regions not in [1, 16]", R);
  RegionOrder order;
  if (region_order_from_host("seg3d_finalize_regions", order_host, R, &order) != SEG3D_OK) return SEG3D_ERR_INVALID;
  RegionOrderBytes bytes;
  for (int r = 0; r < 16; ++r) bytes.v[r] = (signed char)(r < R ? order_host[r] : 0);
  hipLaunchKernelGGL(finalize_regions_kernel, dim3(seg3d_ew_grid(voxels, 256)), dim3(256), 0, (hipStream_t)stream, acc, count,
                     mask, R, bytes, (i64)voxels, (i64)(class_stride ? class_stride : voxels));
  SEG3D_LAUNCH_CHECK("seg3d_finalize_regions");
  return SEG3D_OK;
}
