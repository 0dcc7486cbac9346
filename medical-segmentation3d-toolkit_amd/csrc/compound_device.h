// compound_device.h -- the device code of the compound loss (loss.hip) that the Dice + top-k loss (topk_loss.hip) shares:
// the counting rule, the per-voxel soft-Dice sums, the partial-sum layout, the fp64 finalize rule of the region term and
// the per-voxel gradient.  Definitions: loss.hip ("compound loss") and DESIGN.md section 7, rows f7 and f15.
#pragma once
#include "seg3d_common.h"

#define SEG3D_MAXC 16
#define DICE_VPB 4096  // voxels per workgroup of the Dice / compound partial-sum passes

#define COMPOUND_EPS 1e-5
#define COMPOUND_PMIN 1e-12f

__device__ __forceinline__ float focal_pow(float q, float gamma) {
  if (gamma == 2.0f) return q * q;
  if (gamma == 1.0f) return q;
  return powf(q, gamma);
}

template <int CT>
struct CompoundAcc {
  float r[3 * CT];   // (I, P, T) per class
  float num, den;    // distribution numerator / denominator
};

// (1 - pt)^gamma (-log pt) for pt already clamped; q = max(1 - pt, 0)
__device__ __forceinline__ float compound_dist(float pt, float gamma) {
  const float nl = -logf(pt);
  if (gamma == 0.0f) return nl;
  return focal_pow(fmaxf(1.0f - pt, 0.0f), gamma) * nl;
}

// d/dpt of the above:  gamma q^(gamma-1) log pt - q^gamma / pt   (q = 0: the first product's limit is 0 for every gamma > 0)
__device__ __forceinline__ float compound_dist_grad(float pt, float gamma) {
  if (gamma == 0.0f) return -1.0f / pt;
  const float q = fmaxf(1.0f - pt, 0.0f), lp = logf(pt);
  float qg1;
  if (gamma == 2.0f) qg1 = q;
  else if (gamma == 1.0f) qg1 = 1.0f;
  else qg1 = q > 0.0f ? powf(q, gamma - 1.0f) : 0.0f;
  return gamma * qg1 * lp - focal_pow(q, gamma) / pt;
}

// The counting rule and the region sums of one voxel.  Returns whether the voxel counts; if it does, (I, P, T) of every
// class have taken it and pt / at are the probability and the class weight of its target class.
template <int CT>
__device__ __forceinline__ bool compound_region_voxel(CompoundAcc<CT>& a, float t, const float (&p)[CT],
                                                      const float (&alpha)[CT], int C, float ignore, float& pt, float& at) {
  const bool valid = t >= 0.0f && t < (float)C && t != ignore;
  if (!valid) return false;
  const int ti = (int)t;
  pt = 0.f;
  at = 0.f;
#pragma unroll
  for (int c = 0; c < CT; ++c)
    if (CT <= 5 || c < C) {
      const bool is = ti == c;
      a.r[3 * c + 0] += is ? p[c] : 0.f;
      a.r[3 * c + 1] += p[c];
      a.r[3 * c + 2] += is ? 1.f : 0.f;
      pt = is ? p[c] : pt;
      at = is ? alpha[c] : at;
    }
  return true;
}

template <int CT>
__device__ __forceinline__ void compound_voxel(CompoundAcc<CT>& a, float t, const float (&p)[CT], const float (&alpha)[CT],
                                               int C, float ignore, float gamma) {
  float pt, at;
  if (!compound_region_voxel<CT>(a, t, p, alpha, C, ignore, pt, at)) return;
  a.num += at * compound_dist(fmaxf(pt, COMPOUND_PMIN), gamma);
  a.den += at;
}

// The region term's finalize rule over part[n][blk][3C + 2] (the (I, P, T) triples; the last two slots are not read):
// fp64, fixed order, one 256-thread workgroup, every thread calls.  As in dice_finalize_kernel, 32 lanes per region item
// -- (n, c) over the sample's nblk blocks, or with batch_dice c over all N * nblk blocks -- and a fixed-shape shuffle tree.
// Writes coef[R][C][2] = (A, B) (R = batch_dice ? 1 : N) and returns L_region, valid in thread 0.  `red`: 8 doubles of LDS
// that no thread still reads.
__device__ __forceinline__ double compound_region_finalize(const float* __restrict__ part, const float* __restrict__ wdice,
                                                           float* __restrict__ coef, int N, int C, int nblk, int batch_dice,
                                                           float dice_weight, double* red) {
  const int NV = 3 * C + 2;
  const i64 nent = (i64)N * nblk;
  const int grp = threadIdx.x >> 5, l32 = threadIdx.x & 31;
  const int R = batch_dice ? 1 : N;
  const i64 cnt = batch_dice ? nent : (i64)nblk;
  const double k = batch_dice ? 1.0 : 1.0 / (double)N;
  double acc = 0.0;
  for (int idx0 = 0; idx0 < R * C; idx0 += 8) {   // uniform trip count: the shuffles below need whole waves
    const int idx = idx0 + grp;
    const bool ok = idx < R * C;
    const int r = ok ? idx / C : 0, c = ok ? idx % C : 0;
    double I = 0.0, P = 0.0, T = 0.0;
    if (ok) {
      const float* p = part + (i64)r * nblk * NV + 3 * c;
      for (i64 m = l32; m < cnt; m += 32) {
        I += (double)p[m * NV + 0];
        P += (double)p[m * NV + 1];
        T += (double)p[m * NV + 2];
      }
    }
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) {   // within the 32-lane group
      I += __shfl_down(I, off, 32);
      P += __shfl_down(P, off, 32);
      T += __shfl_down(T, off, 32);
    }
    if (ok && l32 == 0) {
      const double w = (double)wdice[c];
      const double U = P + T + COMPOUND_EPS, nu = 2.0 * I + COMPOUND_EPS;
      acc += w * k * (1.0 - nu / U);
      const bool on = dice_weight > 0.f && w > 0.0;
      coef[2 * idx + 0] = on ? (float)(-(double)dice_weight * w * k * 2.0 / U) : 0.f;
      coef[2 * idx + 1] = on ? (float)((double)dice_weight * w * k * nu / (U * U)) : 0.f;
    }
  }
  if (l32 == 0) red[grp] = acc;
  __syncthreads();
  double lr = 0.0;
  if (threadIdx.x == 0)
    for (int g = 0; g < 8; ++g) lr += red[g];
  return lr;
}

// one voxel's C gradients; g[c] is written for every c < C.  `cd` multiplies the distribution part of this voxel.
template <int CT>
__device__ __forceinline__ void compound_voxel_grad(float (&g)[CT], float t, float pt_in, const float (&A)[CT],
                                                    const float (&B)[CT], const float (&alpha)[CT], int C, float ignore,
                                                    float gamma, float cd, float go) {
  const bool valid = t >= 0.0f && t < (float)C && t != ignore;
  const int ti = valid ? (int)t : -1;
  float dt = 0.f;
  if (valid && cd != 0.f && pt_in >= COMPOUND_PMIN) dt = cd * compound_dist_grad(pt_in, gamma);
#pragma unroll
  for (int c = 0; c < CT; ++c)
    if (CT <= 5 || c < C) {
      const bool is = ti == c;
      const float d = (is ? A[c] + B[c] : B[c]) + (is ? alpha[c] * dt : 0.f);
      g[c] = valid ? go * d : 0.f;
    }
}

static inline bool compound_vec_ok(long long S, const void* a, const void* b, const void* c) {
  return S % 4 == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

#define COMPOUND_DISPATCH(KERNEL, C, vec, ...)                                         \
  do {                                                                                 \
    switch (C) {                                                                       \
      case 1: if (vec) KERNEL<1, true> __VA_ARGS__; else KERNEL<1, false> __VA_ARGS__; break;    \
      case 2: if (vec) KERNEL<2, true> __VA_ARGS__; else KERNEL<2, false> __VA_ARGS__; break;    \
      case 3: if (vec) KERNEL<3, true> __VA_ARGS__; else KERNEL<3, false> __VA_ARGS__; break;    \
      case 4: if (vec) KERNEL<4, true> __VA_ARGS__; else KERNEL<4, false> __VA_ARGS__; break;    \
      case 5: if (vec) KERNEL<5, true> __VA_ARGS__; else KERNEL<5, false> __VA_ARGS__; break;    \
      default: if (vec) KERNEL<SEG3D_MAXC, true> __VA_ARGS__; else KERNEL<SEG3D_MAXC, false> __VA_ARGS__; break; \
    }                                                                                  \
  } while (0)
