// compound_device.h -- what the compound loss family shares: Dice + CE / focal (loss.hip), Dice + top-k (topk_loss.hip),
// Dice + boundary (boundary_loss.hip), Dice + clDice (cldice_loss.hip) and the region loss on sigmoid planes (region_loss.hip:
// planes as classes, its own per-voxel rule); validation.hip takes the counting rule.
// Definitions: loss.hip ("compound loss") and DESIGN.md section 7, rows f7, f15, f16, f17 and f23.
//
// Every loss of the family streams probs [N][C][S] and target [N][S] once, forward and backward:
//   counting rule  a voxel counts iff 0 <= t < C && t != ignore; its class is (int)t  (compound_class)
//   CT, VEC        CT is the compile-time class count (1..5: exact, accumulators in registers; 16: generic, planes c >= C
//                  predicated off).  VEC: S % 4 == 0 and 16-byte aligned bases -> W = 4 consecutive voxels per lane and
//                  access, else W = 1  (compound_load / compound_store, COMPOUND_DISPATCH)
//   forward        grid (ceil(S / DICE_VPB), N), 256 threads: workgroup (blk, n) owns voxels [blk * DICE_VPB, + DICE_VPB) of
//                  sample n; thread i takes s = s0 + i W, s0 + (256 + i) W, ... and the W voxels of an access in address
//                  order  (compound_block_walk).  part[n][blk][3C + 2] = the block's (I, P, T) per class, written by
//                  compound_region_store, then two slots of the caller (compound loss: distribution numerator and
//                  denominator; the others: 0).  The soft-Dice term of every loss is this one code, so it is the same number.
//   finalize       one 256-thread workgroup, fp64, fixed order  (compound_column_sum, compound_region_finalize)
//   backward       grid compound_bwd_grid(S, N, vec) = (blocks, N), grid-stride over the sample's voxels; coef[R][C][2] = (A, B) of the
//                  region term (R = batch_dice ? 1 : N), then the loss's own coefficients  (compound_load_coef,
//                  compound_bwd_body)
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
  float r[3 * CT] = {};         // (I, P, T) per class
  float num = 0.f, den = 0.f;   // distribution numerator / denominator
};

// the counting rule: the class id of a target value, -1 if the voxel does not count
__device__ __forceinline__ int compound_class(float t, int C, float ignore) {
  const bool valid = t >= 0.0f && t < (float)C && t != ignore;
  return valid ? (int)t : -1;
}

// W consecutive floats: W = 4 is one 16-byte access (the caller guarantees the alignment), W = 1 a scalar one
template <int W>
__device__ __forceinline__ void compound_load(float (&v)[W], const float* p) {
  static_assert(W == 1 || W == 4, "one scalar or one 16-byte access");
  if constexpr (W == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    v[0] = p[0];
  }
}
template <int W>
__device__ __forceinline__ void compound_store(float* p, const float (&v)[W]) {
  static_assert(W == 1 || W == 4, "one scalar or one 16-byte access");
  if constexpr (W == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else p[0] = v[0];
}

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
  const int ti = compound_class(t, C, ignore);
  if (ti < 0) return false;
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

// The forward walk of workgroup (blockIdx.x, blockIdx.y = n) over its DICE_VPB voxels of sample n.  body(s, t, p) gets
// the W targets at s .. s + W - 1 and p[j][c], the probability of class c at voxel s + j (0 for c >= C), and consumes
// j = 0 .. W - 1 in that order: the thread-to-voxel map and the order of a thread's additions are the same for every loss.
template <int CT, int W, typename Body>
__device__ __forceinline__ void compound_block_walk(const float* __restrict__ probs, const float* __restrict__ target, int C,
                                                    i64 S, Body&& body) {
  const i64 s0 = (i64)blockIdx.x * DICE_VPB;
  i64 s1 = s0 + DICE_VPB;
  if (s1 > S) s1 = S;
  const float* tg = target + (i64)blockIdx.y * S;
  const float* pb = probs + (i64)blockIdx.y * C * S;
  for (i64 s = s0 + (i64)threadIdx.x * W; s < s1; s += 256 * W) {   // W = 4: S % 4 == 0, so s1 is a multiple of 4
    float t[W], plane[CT][W], p[W][CT];
    compound_load<W>(t, tg + s);
#pragma unroll
    for (int c = 0; c < CT; ++c)
      if (CT <= 5 || c < C) compound_load<W>(plane[c], pb + (i64)c * S + s);
#pragma unroll
    for (int j = 0; j < W; ++j)
#pragma unroll
      for (int c = 0; c < CT; ++c) p[j][c] = (CT <= 5 || c < C) ? plane[c][j] : 0.f;
    body(s, t, p);
  }
}

// The workgroup's (I, P, T) sums into its part[n][blk][3C + 2] entry; returns the entry, whose last two slots thread 0 of
// the caller writes.  `red`: 12 floats of LDS.
template <int CT>
__device__ __forceinline__ float* compound_region_store(const CompoundAcc<CT>& a, float* __restrict__ part, int C, int nblk,
                                                        float* red) {
  float* dst = part + ((i64)blockIdx.y * nblk + blockIdx.x) * (3 * C + 2);
#pragma unroll
  for (int c = 0; c < CT; ++c)
    if (CT <= 5 || c < C) {
      float v[3] = {a.r[3 * c + 0], a.r[3 * c + 1], a.r[3 * c + 2]};
      block_sum_256<3>(v, red);
      if (threadIdx.x == 0) { dst[3 * c + 0] = v[0]; dst[3 * c + 1] = v[1]; dst[3 * c + 2] = v[2]; }
    }
  return dst;
}

// v[k] = fp64 sum of col[k], col[stride + k], ... (cnt terms) for NC adjacent columns by one 256-thread workgroup in fixed
// order: thread i adds terms i, i + 256, ..., then a wave64 shuffle tree, then the four waves in order.  Every thread calls
// and gets the totals.  `red`: 4 * NC doubles of LDS that no thread still reads; free again on return.
template <int NC, typename T>
__device__ __forceinline__ void compound_column_sum(double (&v)[NC], const T* __restrict__ col, i64 cnt, i64 stride,
                                                    double* red) {
#pragma unroll
  for (int k = 0; k < NC; ++k) v[k] = 0.0;
  for (i64 m = threadIdx.x; m < cnt; m += 256) {
#pragma unroll
    for (int k = 0; k < NC; ++k) v[k] += (double)col[m * stride + k];
  }
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    v[k] = wave_sum_d(v[k]);
    if ((threadIdx.x & 63) == 0) red[4 * k + (threadIdx.x >> 6)] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NC; ++k) v[k] = red[4 * k + 0] + red[4 * k + 1] + red[4 * k + 2] + red[4 * k + 3];
  __syncthreads();
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
  const int ti = compound_class(t, C, ignore);
  const bool valid = ti >= 0;
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

// (A, B) of coefficient row r and the loss's own per-class factor x[c] = row[c]; all 0 for c >= C
template <int CT>
__device__ __forceinline__ void compound_load_coef(float (&A)[CT], float (&B)[CT], float (&x)[CT], const float* coef, int r,
                                                   const float* row, int C) {
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    const bool on = CT <= 5 || c < C;
    A[c] = on ? coef[2 * (r * C + c) + 0] : 0.f;
    B[c] = on ? coef[2 * (r * C + c) + 1] : 0.f;
    x[c] = on ? row[c] : 0.f;
  }
}

// The backward of a loss whose distribution part is a per-voxel multiple of compound_dist: grid (blocks, N), so the sample
// -- and with it the coefficient row -- is uniform per workgroup.  dist_coef(s, cd) fills cd[j], the multiplier of voxel
// s + j.  With 16-byte accesses and few classes every plane is loaded and p_t picked in registers; otherwise each voxel
// gathers the one probability it needs.
template <int CT, int W, typename DistCoef>
__device__ __forceinline__ void compound_bwd_body(const float* __restrict__ probs, const float* __restrict__ target,
                                                  const float* __restrict__ coef, const float* __restrict__ alpha_g,
                                                  const float* __restrict__ gout, float* __restrict__ dprobs, int C, i64 S,
                                                  int R, float ignore, float gamma, DistCoef&& dist_coef) {
  const int n = blockIdx.y;
  const float go = gout[0];
  float A[CT], B[CT], alpha[CT];
  compound_load_coef<CT>(A, B, alpha, coef, R == 1 ? 0 : n, alpha_g, C);
  const float* tg = target + (i64)n * S;
  const float* pb = probs + (i64)n * C * S;
  float* db = dprobs + (i64)n * C * S;
  for (i64 s = ((i64)blockIdx.x * 256 + threadIdx.x) * W; s < S; s += (i64)gridDim.x * 256 * W) {
    float t[W], cd[W], pt[W], g[W][CT];
    compound_load<W>(t, tg + s);
    dist_coef(s, cd);
#pragma unroll
    for (int j = 0; j < W; ++j) pt[j] = 0.f;
    if constexpr (CT <= 5 && W == 4) {
      int ti[W];   // the class of the counting rule, (int)t: a target such as 1.7 selects p_1, as in the forward
#pragma unroll
      for (int j = 0; j < W; ++j) ti[j] = compound_class(t[j], C, ignore);
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        float p[W];
        compound_load<W>(p, pb + (i64)c * S + s);
#pragma unroll
        for (int j = 0; j < W; ++j) pt[j] = ti[j] == c ? p[j] : pt[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < W; ++j)
        if (t[j] >= 0.0f && t[j] < (float)C) pt[j] = pb[(i64)(int)t[j] * S + s + j];
    }
#pragma unroll
    for (int j = 0; j < W; ++j) compound_voxel_grad<CT>(g[j], t[j], pt[j], A, B, alpha, C, ignore, gamma, cd[j], go);
#pragma unroll
    for (int c = 0; c < CT; ++c)
      if (CT <= 5 || c < C) {
        float gc[W];
#pragma unroll
        for (int j = 0; j < W; ++j) gc[j] = g[j][c];
        compound_store<W>(db + (i64)c * S + s, gc);
      }
  }
}

static inline bool compound_vec_ok(long long S, const void* a, const void* b, const void* c) {
  return S % 4 == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

// the backward grid (blocks, N) over S voxels of each of N samples: one access per thread, at most 8192 workgroups in all
static inline dim3 compound_bwd_grid(long long S, int N, bool vec) {
  const i64 items = vec ? S / 4 : S;
  i64 gx = (items + 255) / 256, cap = 8192 / N;
  if (cap < 1) cap = 1;
  if (gx > cap) gx = cap;
  return dim3((unsigned)gx, (unsigned)N);
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
