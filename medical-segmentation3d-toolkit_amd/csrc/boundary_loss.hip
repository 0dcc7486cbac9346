// boundary_loss.hip -- boundary (signed-distance) loss of Kervadec et al. (MIDL 2019) next to the compound loss's soft-Dice
// term, with the dense batched signed Euclidean distance map computed on the device (no counterpart in the reference;
// definitions in DESIGN.md section 7, row f16, and include/seg3d_hip.h).
//   counted voxel:  the compound loss family's rule (compound_device.h)
//   for sample n and class c:  G = counted voxels with (int)t == c,  H = counted voxels with (int)t != c
//   phi[n,c](v) = +d(v, G) on H,  -d(v, H) on G,  0 on voxels that do not count and wherever G or H is empty
//   d = Euclidean distance of voxel centres in physical units; plain edt(~m) - edt(m), no "- 1" offset
//   L_boundary = sum_c w'_c (sum_{n, counted v} phi[n,c](v) p[n,c](v)) / max(1, n_counted)
//   L = dice_weight L_region + boundary_weight L_boundary,  L_region = the compound loss's soft-Dice term
//   dL/dp[n,c,v] = (A t_c + B) + boundary_weight w'_c phi[n,c](v) / max(1, n_counted) on counted voxels, 0 elsewhere
//
// Distance map: three separable passes of the exact squared transform, out(u) = min_i f(i) + w^2 (u - i)^2, evaluated by
// brute force over the whole line (lines are at most 256 long).  No stacks, no data-dependent loops or addresses:
//   pass x  reads the target row into LDS as class codes (one wave per row, lane u + 64 j) and writes BOTH transforms --
//           features G and features H -- from that one load; a row voxel is a feature of exactly one of them, and the
//           code is wave-uniform, so each step updates one set of accumulators;
//   pass y / z  stage a tile of 32 neighbouring lines x L of both fields in LDS ([field][i][lane]: lanes read consecutive
//           banks, the eight line segments of a workgroup read the same addresses) and compute four outputs per thread and
//           LDS read; in place (a workgroup owns its lines); pass z writes phi = +sqrt / -sqrt / 0 by the voxel's target.
// "No feature" is the sentinel SDF_NONE = 1e30: spacing <= 1e6 keeps every real squared distance below 2e17 and every
// w^2 (u - i)^2 below half an ulp of the sentinel, so sentinel + anything real == sentinel: no overflow, no inf - inf.
// With unit spacing every intermediate is an integer below 2^24: the squared distances are exact.
#include "seg3d_common.h"
#include "seg3d_hip.h"
#include "compound_device.h"

#define SDF_NONE 1e30f
#define SDF_MAX_AXIS 256
#define SDF_TILE 32            // neighbouring lines per workgroup of pass y / z
#define SDF_MAX_SPACING 1e6
#define SDF_MIN_SPACING 1e-6

// pass x: field[n][k][0 / 1][z][y][x] = squared distance along the row to the nearest G / H voxel (SDF_NONE: none).
// grid (rows / 4, K); one wave per row, lane handles u = lane + 64 j, j < J.
template <int J>
__global__ __launch_bounds__(256) void sdf_x_kernel(const float* __restrict__ target, float* __restrict__ field, int X,
                                                      i64 rows, i64 rows_per_sample, i64 S, int K, Seg3dClassList cls, int C,
                                                      float ignore, float w) {
  __shared__ int code[4][SDF_MAX_AXIS];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const i64 row = (i64)blockIdx.x * 4 + wave;
  const bool active = row < rows;
  const int k = blockIdx.y;
  const int c = cls.id[k];
  if (active) {
    const float* tr = target + row * X;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int u = lane + 64 * j;
      if (u < X) code[wave][u] = compound_class(tr[u], C, ignore);
    }
  }
  __syncthreads();
  if (!active) return;
  float g[J], h[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    g[j] = SDF_NONE;
    h[j] = SDF_NONE;
  }
  for (int i = 0; i < X; ++i) {
    const int ci = __builtin_amdgcn_readfirstlane(code[wave][i]);   // the same word for the whole wave
    if (ci < 0) continue;
    if (ci == c) {
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const float d = (float)(lane + 64 * j - i);
        g[j] = fminf(g[j], d * d * w);
      }
    } else {
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const float d = (float)(lane + 64 * j - i);
        h[j] = fminf(h[j], d * d * w);
      }
    }
  }
  const i64 n = row / rows_per_sample;
  float* fg = field + ((n * K + k) * 2) * S + (row - n * rows_per_sample) * X;
  float* fh = fg + S;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int u = lane + 64 * j;
    if (u < X) {
      fg[u] = g[j];
      fh[u] = h[j];
    }
  }
}

// pass y / z over both fields of one (n, k): lines of length L with element stride `inner`; `outer` blocks of L * inner
// elements per field (pass y: outer = Z, inner = X; pass z: outer = 1, inner = Y * X).
// grid (outer * tiles, N * K), tiles = ceil(inner / 32); dynamic LDS 2 * L * 32 floats.
template <bool FINAL>
__global__ __launch_bounds__(256) void sdf_line_kernel(float* __restrict__ field, const float* __restrict__ target,
                                                         float* __restrict__ phi, int L, i64 inner, int tiles, i64 S, int K,
                                                         Seg3dClassList cls, int C, float ignore, float w) {
  extern __shared__ float lds[];
  float* lg = lds;
  float* lh = lds + L * SDF_TILE;
  const int tx = threadIdx.x & (SDF_TILE - 1), ug = threadIdx.x / SDF_TILE;   // ug: 0..7
  const int nk = blockIdx.y;
  const i64 o = blockIdx.x / tiles;
  const i64 x = (i64)(blockIdx.x % tiles) * SDF_TILE + tx;
  const bool in = x < inner;
  const i64 base = o * L * inner + x;              // within one field / one sample's volume
  float* fg = field + ((i64)nk * 2) * S + base;
  float* fh = fg + S;
  for (int i = ug; i < L; i += 256 / SDF_TILE) {
    lg[i * SDF_TILE + tx] = in ? fg[(i64)i * inner] : SDF_NONE;
    lh[i * SDF_TILE + tx] = in ? fh[(i64)i * inner] : SDF_NONE;
  }
  __syncthreads();
  for (int u0 = ug * 4; u0 < L; u0 += 4 * (256 / SDF_TILE)) {
    float g[4] = {SDF_NONE, SDF_NONE, SDF_NONE, SDF_NONE}, h[4] = {SDF_NONE, SDF_NONE, SDF_NONE, SDF_NONE};
#pragma unroll 4
    for (int i = 0; i < L; ++i) {
      const float a = lg[i * SDF_TILE + tx], b = lh[i * SDF_TILE + tx];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d = (float)(u0 + j - i);
        const float dd = d * d;
        g[j] = fminf(g[j], fmaf(dd, w, a));
        h[j] = fminf(h[j], fmaf(dd, w, b));
      }
    }
    if (!in) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int u = u0 + j;
      if (u >= L) continue;
      const float gv = fminf(g[j], SDF_NONE), hv = fminf(h[j], SDF_NONE);
      if constexpr (FINAL) {
        const int n = nk / K, c = cls.id[nk % K];
        const int ct = compound_class(target[(i64)n * S + base + (i64)u * inner], C, ignore);
        float v = 0.f;
        if (ct >= 0) {
          const float q = ct == c ? hv : gv;          // a G voxel asks for H, an H voxel for G
          if (q < 0.5f * SDF_NONE) v = ct == c ? -sqrtf(q) : sqrtf(q);
        }
        phi[(i64)nk * S + base + (i64)u * inner] = v;
      } else {
        fg[(i64)u * inner] = gv;
        fh[(i64)u * inner] = hv;
      }
    }
  }
}

extern "C" long long seg3d_signed_distance_workspace_bytes(int N, int K, int X, int Y, int Z) {
  if (N <= 0 || K <= 0 || X <= 0 || Y <= 0 || Z <= 0) return 0;
  return (long long)N * K * 2 * X * Y * Z * 4;
}

extern "C" int seg3d_signed_distance(const float* target, float* phi, void* workspace, int N, int X, int Y, int Z,
                                     Seg3dClassList class_ids, int K, int num_class, double sx, double sy, double sz,
                                     float ignore_label, void* stream) {
  SEG3D_REQUIRE(target && phi && workspace && N > 0, "seg3d_signed_distance: bad arguments");
  SEG3D_REQUIRE(X >= 1 && X <= SDF_MAX_AXIS && Y >= 1 && Y <= SDF_MAX_AXIS && Z >= 1 && Z <= SDF_MAX_AXIS,
                "seg3d_signed_distance: every axis of (%d, %d, %d) must be in [1, %d]", X, Y, Z, SDF_MAX_AXIS);
  SEG3D_REQUIRE(K >= 1 && K <= SEG3D_MAXC, "seg3d_signed_distance: %d class ids, not in [1, %d]", K, SEG3D_MAXC);
  SEG3D_REQUIRE(num_class >= 1 && num_class <= (1 << 24), "seg3d_signed_distance: num_class %d not in [1, 2^24]", num_class);
  SEG3D_REQUIRE(sx >= SDF_MIN_SPACING && sx <= SDF_MAX_SPACING && sy >= SDF_MIN_SPACING && sy <= SDF_MAX_SPACING &&
                    sz >= SDF_MIN_SPACING && sz <= SDF_MAX_SPACING,
                "seg3d_signed_distance: spacing (%g, %g, %g) not in [1e-6, 1e6]", sx, sy, sz);   // NaN fails the comparisons
  SEG3D_REQUIRE((i64)N * K <= 65535, "seg3d_signed_distance: N * K = %lld above 65535", (i64)N * K);
  const i64 S = (i64)X * Y * Z;
  SEG3D_REQUIRE((i64)N * S < (1ll << 31), "seg3d_signed_distance: N * S = %lld not below 2^31", (i64)N * S);
  hipStream_t s = (hipStream_t)stream;
  float* field = reinterpret_cast<float*>(workspace);
  const float wx = (float)(sx * sx), wy = (float)(sy * sy), wz = (float)(sz * sz);
  const i64 rows = (i64)N * Z * Y, rps = (i64)Z * Y;
  const dim3 gx((unsigned)((rows + 3) / 4), K);
  switch ((X + 63) / 64) {
    case 1: sdf_x_kernel<1><<<gx, dim3(256), 0, s>>>(target, field, X, rows, rps, S, K, class_ids, num_class, ignore_label, wx); break;
    case 2: sdf_x_kernel<2><<<gx, dim3(256), 0, s>>>(target, field, X, rows, rps, S, K, class_ids, num_class, ignore_label, wx); break;
    case 3: sdf_x_kernel<3><<<gx, dim3(256), 0, s>>>(target, field, X, rows, rps, S, K, class_ids, num_class, ignore_label, wx); break;
    default: sdf_x_kernel<4><<<gx, dim3(256), 0, s>>>(target, field, X, rows, rps, S, K, class_ids, num_class, ignore_label, wx); break;
  }
  SEG3D_LAUNCH_CHECK("seg3d_signed_distance(x)");
  {
    const int tiles = (X + SDF_TILE - 1) / SDF_TILE;
    sdf_line_kernel<false><<<dim3((unsigned)(Z * tiles), N * K), dim3(256), (size_t)2 * Y * SDF_TILE * 4, s>>>(
        field, target, phi, Y, (i64)X, tiles, S, K, class_ids, num_class, ignore_label, wy);
    SEG3D_LAUNCH_CHECK("seg3d_signed_distance(y)");
  }
  {
    const i64 inner = (i64)X * Y;
    const int tiles = (int)((inner + SDF_TILE - 1) / SDF_TILE);
    sdf_line_kernel<true><<<dim3((unsigned)tiles, N * K), dim3(256), (size_t)2 * Z * SDF_TILE * 4, s>>>(
        field, target, phi, Z, inner, tiles, S, K, class_ids, num_class, ignore_label, wz);
    SEG3D_LAUNCH_CHECK("seg3d_signed_distance(z)");
  }
  return SEG3D_OK;
}

// ---- the loss ----------------------------------------------------------------------------------------------------------
// Forward pass A: the (I, P, T) triples of part (its two trailing slots are 0) and, by the same walk, bpart[n][blk][C + 1] =
// per class sum phi p over the block's counted voxels (0 for an excluded background), then the number of counted voxels.
// phi: [N][C - c0][S], c0 = 0 with the background, 1 without.
template <int CT>
__device__ __forceinline__ void boundary_voxel(CompoundAcc<CT>& a, float (&b)[CT], float& cnt, float t, const float (&p)[CT],
                                               const float (&ph)[CT], const float (&zero)[CT], int C, float ignore) {
  float pt, at;
  if (!compound_region_voxel<CT>(a, t, p, zero, C, ignore, pt, at)) return;
  cnt += 1.0f;
#pragma unroll
  for (int c = 0; c < CT; ++c)
    if (CT <= 5 || c < C) b[c] = fmaf(ph[c], p[c], b[c]);
}

template <int CT, bool VEC>
__global__ __launch_bounds__(256) void boundary_partial_kernel(const float* __restrict__ probs, const float* __restrict__ target,
                                                                 const float* __restrict__ phi, float* __restrict__ part,
                                                                 float* __restrict__ bpart, int C, int c0, i64 S, int nblk,
                                                                 float ignore) {
  constexpr int W = VEC ? 4 : 1;
  __shared__ float red[4 * 3];
  const float* hb = phi + (i64)blockIdx.y * (C - c0) * S;   // plane of class c >= c0 at hb + (c - c0) * S
  float zero[CT] = {}, b[CT] = {};
  float cnt = 0.f;
  CompoundAcc<CT> a;
  compound_block_walk<CT, W>(probs, target, C, S, [&](i64 s, const float (&t)[W], const float (&p)[W][CT]) {
    float plane[CT][W] = {};
#pragma unroll
    for (int c = 0; c < CT; ++c)
      if ((CT <= 5 || c < C) && c >= c0) compound_load<W>(plane[c], hb + (i64)(c - c0) * S + s);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      float ph[CT];
#pragma unroll
      for (int c = 0; c < CT; ++c) ph[c] = plane[c][j];
      boundary_voxel<CT>(a, b, cnt, t[j], p[j], ph, zero, C, ignore);
    }
  });
  float* dst = compound_region_store<CT>(a, part, C, nblk, red);
  float* bdst = bpart + ((i64)blockIdx.y * nblk + blockIdx.x) * (C + 1);
#pragma unroll
  for (int c = 0; c < CT; ++c)
    if (CT <= 5 || c < C) {
      float q[1] = {b[c]};
      block_sum_256<1>(q, red);
      if (threadIdx.x == 0) bdst[c] = q[0];
    }
  float q[1] = {cnt};
  block_sum_256<1>(q, red);
  if (threadIdx.x == 0) {
    bdst[C] = q[0];
    dst[3 * C + 0] = 0.f;
    dst[3 * C + 1] = 0.f;
  }
}

// One workgroup, fp64, fixed order: the C + 1 boundary sums over all N * nblk blocks (threads stride over the blocks, a
// fixed shuffle tree, the four waves in order), then the compound loss's region rule.  loss[3] = (L, L_region,
// L_boundary); coef: [R][C][2] = (A, B), then per class boundary_weight * w'_c / max(1, n_counted).
__global__ __launch_bounds__(256) void boundary_finalize_kernel(const float* __restrict__ part, const float* __restrict__ bpart,
                                                                  const float* __restrict__ wdice,
                                                                  const float* __restrict__ bweight, float* __restrict__ coef,
                                                                  float* __restrict__ loss, int N, int C, int nblk,
                                                                  int batch_dice, float dice_weight) {
  __shared__ double red[8];
  __shared__ double tot[SEG3D_MAXC + 1];
  const i64 nent = (i64)N * nblk;
  for (int c = 0; c <= C; ++c) {
    double v[1];
    compound_column_sum(v, bpart + c, nent, C + 1, red);
    if (threadIdx.x == 0) tot[c] = v[0];
  }
  const double lr = compound_region_finalize(part, wdice, coef, N, C, nblk, batch_dice, dice_weight, red);
  if (threadIdx.x == 0) {
    const double bw = (double)bweight[0];
    const double ncnt = tot[C] > 1.0 ? tot[C] : 1.0;
    const int R = batch_dice ? 1 : N;
    double lb = 0.0;
    for (int c = 0; c < C; ++c) {
      const double w = (double)wdice[c];
      lb += w * tot[c];
      coef[2 * R * C + c] = (float)(bw * w / ncnt);
    }
    lb /= ncnt;
    double l = bw * lb;
    if (dice_weight > 0.f) l += (double)dice_weight * lr;
    loss[0] = (float)l;
    loss[1] = (float)lr;
    loss[2] = (float)lb;
  }
}

// grid (blocks, N); all C planes in one pass; reads the target, the C - c0 phi planes and the coefficient block
template <int CT, bool VEC>
__global__ __launch_bounds__(256) void boundary_bwd_kernel(const float* __restrict__ target, const float* __restrict__ phi,
                                                             const float* __restrict__ coef, const float* __restrict__ gout,
                                                             float* __restrict__ dprobs, int C, int c0, i64 S, int R,
                                                             float ignore) {
  constexpr int W = VEC ? 4 : 1;
  const int n = blockIdx.y;
  const float go = gout[0];
  float A[CT], B[CT], bw[CT];
  compound_load_coef<CT>(A, B, bw, coef, R == 1 ? 0 : n, coef + 2 * R * C, C);
  if (c0 > 0) bw[0] = 0.f;
  const float* tg = target + (i64)n * S;
  const float* hb = phi + (i64)n * (C - c0) * S;
  float* db = dprobs + (i64)n * C * S;
  for (i64 s = ((i64)blockIdx.x * 256 + threadIdx.x) * W; s < S; s += (i64)gridDim.x * 256 * W) {
    float t[W];
    compound_load<W>(t, tg + s);
    int ti[W];
#pragma unroll
    for (int j = 0; j < W; ++j) ti[j] = compound_class(t[j], C, ignore);
#pragma unroll
    for (int c = 0; c < CT; ++c)
      if (CT <= 5 || c < C) {
        float h[W] = {}, g[W];
        if (c >= c0) compound_load<W>(h, hb + (i64)(c - c0) * S + s);
#pragma unroll
        for (int j = 0; j < W; ++j) g[j] = ti[j] >= 0 ? go * fmaf(bw[c], h[j], ti[j] == c ? A[c] + B[c] : B[c]) : 0.f;
        compound_store<W>(db + (i64)c * S + s, g);
      }
  }
}

// Dice partial sums | boundary partial sums
extern "C" long long seg3d_boundary_loss_workspace_bytes(int N, int C, long long S) {
  if (N <= 0 || C <= 0 || S <= 0) return 0;
  return (seg3d_compound_loss_part_floats(N, C, S) + (long long)N * seg3d_dice_blocks(S) * (C + 1)) * 4;
}

extern "C" int seg3d_boundary_loss_fwd(const float* probs, const float* target, const float* phi, const float* wdice,
                                       const float* boundary_weight, void* workspace, float* coef, float* loss, int N, int C,
                                       long long S, float dice_weight, int include_background, int batch_dice,
                                       float ignore_label, void* stream) {
  SEG3D_REQUIRE(probs && target && phi && wdice && boundary_weight && workspace && coef && loss && N > 0 && N <= 65535 &&
                    S > 0,
                "seg3d_boundary_loss_fwd: bad arguments");
  SEG3D_REQUIRE(C >= 1 && C <= SEG3D_MAXC, "seg3d_boundary_loss_fwd: num_class %d not in [1, %d]", C, SEG3D_MAXC);
  SEG3D_REQUIRE(include_background || C >= 2, "seg3d_boundary_loss_fwd: no class is left without the background");
  SEG3D_REQUIRE(dice_weight >= 0.f, "seg3d_boundary_loss_fwd: dice_weight must be >= 0");
  SEG3D_REQUIRE((i64)N * S < (1ll << 31), "seg3d_boundary_loss_fwd: N * S = %lld not below 2^31", (i64)N * S);
  SEG3D_REQUIRE(((uintptr_t)phi & 15) == 0 && ((uintptr_t)workspace & 3) == 0,
                "seg3d_boundary_loss_fwd: phi must be 16-byte aligned, the workspace 4-byte aligned");
  const int nblk = (int)seg3d_dice_blocks(S);
  float* part = reinterpret_cast<float*>(workspace);
  float* bpart = part + seg3d_compound_loss_part_floats(N, C, S);
  const int c0 = include_background ? 0 : 1;
  const bool vec = compound_vec_ok(S, probs, target, probs);   // the compound loss's own choice: same order of additions
  hipStream_t s = (hipStream_t)stream;
  COMPOUND_DISPATCH(boundary_partial_kernel, C, vec,
                    <<<dim3(nblk, N), dim3(256), 0, s>>>(probs, target, phi, part, bpart, C, c0, (i64)S, nblk, ignore_label));
  SEG3D_LAUNCH_CHECK("seg3d_boundary_loss_fwd(partial)");
  boundary_finalize_kernel<<<dim3(1), dim3(256), 0, s>>>(part, bpart, wdice, boundary_weight, coef, loss, N, C, nblk,
                                                         batch_dice ? 1 : 0, dice_weight);
  SEG3D_LAUNCH_CHECK("seg3d_boundary_loss_fwd(finalize)");
  return SEG3D_OK;
}

extern "C" int seg3d_boundary_loss_bwd(const float* target, const float* phi, const float* coef, const float* gout,
                                       float* dprobs, int N, int C, long long S, int include_background, int batch_dice,
                                       float ignore_label, void* stream) {
  SEG3D_REQUIRE(target && phi && coef && gout && dprobs && N > 0 && N <= 65535 && S > 0, "seg3d_boundary_loss_bwd: bad arguments");
  SEG3D_REQUIRE(C >= 1 && C <= SEG3D_MAXC, "seg3d_boundary_loss_bwd: num_class %d not in [1, %d]", C, SEG3D_MAXC);
  SEG3D_REQUIRE(include_background || C >= 2, "seg3d_boundary_loss_bwd: no class is left without the background");
  SEG3D_REQUIRE((i64)N * S < (1ll << 31), "seg3d_boundary_loss_bwd: N * S = %lld not below 2^31", (i64)N * S);
  const bool vec = compound_vec_ok(S, target, phi, dprobs);
  const int R = batch_dice ? 1 : N;
  const int c0 = include_background ? 0 : 1;
  COMPOUND_DISPATCH(boundary_bwd_kernel, C, vec,
                    <<<compound_bwd_grid(S, N, vec), dim3(256), 0, (hipStream_t)stream>>>(target, phi, coef, gout, dprobs, C,
                                                                                         c0, (i64)S, R, ignore_label));
  SEG3D_LAUNCH_CHECK("seg3d_boundary_loss_bwd");
  return SEG3D_OK;
}
