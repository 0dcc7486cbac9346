// region_loss.hip -- soft Dice + binary cross-entropy / focal on the sigmoid probabilities of a region-based model, forward +
// backward (no counterpart in the reference, which knows exclusive classes only).
//
// probs [N][R][S] planar fp32 (what the sigmoid head writes, 1 <= R <= 16), target [N][S] float label ids, lut[256]: bit r of
// lut[l] says whether label l belongs to region r (loss/region_loss.py region_lut).  Regions may overlap, so every plane has a
// binary target of its own:
//   counting rule  region_device.h: l = label_byte(t), a voxel counts iff l >= 0 && t != ignore.  A voxel that does not
//                  count enters no sum and gets gradient 0 on every plane.  z_r = (lut[l] >> r) & 1: a label in no region is
//                  background for every region.
//   Dice term      the compound family's with planes as classes: I = sum p z, P = sum p, T = sum z over counted voxels,
//                  d[n,r] = (2 I + 1e-5) / (P + T + 1e-5),  L_dice = sum_r w'_r (1 - mean_n d[n,r])   (batch_dice: one ratio
//                  per region over the whole batch).  Partial sums, finalize and (A, B) are compound_device.h's, unchanged.
//   BCE term       q = z ? p : 1 - p,  qc = max(q, 1e-12),  l_r = compound_dist(qc, gamma)  (-log qc at gamma = 0, focal
//                  otherwise: one logarithm per plane and voxel),
//                  L_bce = sum_v sum_r a_r l_r / (n_counted sum_r a_r), 0 when nothing counts.
//   L = dice_weight * L_dice + bce_weight * L_bce; a term whose weight is 0 never enters L.
//   dL/dp[n,r,s] = (z ? A + B : B) + bce_weight a_r / (n_counted sum_r a_r) compound_dist_grad(q, gamma) (z ? 1 : -1) [q >= 1e-12]
// Forward: ONE pass (compound_block_walk) leaves part[n][blk][3R + 2]: the (I, P, T) triples, then the block's BCE numerator
// and its number of counted voxels (<= DICE_VPB, exact in fp32).  A one-workgroup fp64 finalize in fixed order.  No atomics,
// no allocation, no synchronisation: bit-reproducible and capturable.
// HBM-bound: algorithmic bytes per voxel = 4 (R + 1) forward, 4 (2 R + 1) backward.
#include "seg3d_common.h"
#include "seg3d_hip.h"
#include "compound_device.h"
#include "region_device.h"   // RegionLut, region_bits: the table and the counting rule

template <int CT>
__device__ __forceinline__ void region_voxel(CompoundAcc<CT>& a, int bits, const float (&p)[CT], const float (&alpha)[CT],
                                             int R, float gamma) {
  if (bits < 0) return;
#pragma unroll
  for (int r = 0; r < CT; ++r)
    if (CT <= 5 || r < R) {
      const bool z = (bits >> r) & 1;
      a.r[3 * r + 0] += z ? p[r] : 0.f;
      a.r[3 * r + 1] += p[r];
      a.r[3 * r + 2] += z ? 1.f : 0.f;
      const float q = z ? p[r] : 1.0f - p[r];
      a.num += alpha[r] * compound_dist(fmaxf(q, COMPOUND_PMIN), gamma);
    }
  a.den += 1.f;
}

template <int CT, bool VEC>
__global__ __launch_bounds__(256) void region_partial_kernel(const float* __restrict__ probs, const float* __restrict__ target,
                                                               RegionLut table, const float* __restrict__ alpha_g,
                                                               float* __restrict__ part, int R, i64 S, int nblk, float ignore,
                                                               float gamma) {
  constexpr int W = VEC ? 4 : 1;
  __shared__ float red[4 * 3];
  const unsigned* lut = table.stage();
  float alpha[CT];
#pragma unroll
  for (int r = 0; r < CT; ++r) alpha[r] = (CT <= 5 || r < R) ? alpha_g[r] : 0.f;
  CompoundAcc<CT> a;
  compound_block_walk<CT, W>(probs, target, R, S, [&](i64, const float (&t)[W], const float (&p)[W][CT]) {
#pragma unroll
    for (int j = 0; j < W; ++j) region_voxel<CT>(a, region_bits(lut, t[j], ignore), p[j], alpha, R, gamma);
  });
  float* dst = compound_region_store<CT>(a, part, R, nblk, red);
  float v[2] = {a.num, a.den};
  block_sum_256<2>(v, red);
  if (threadIdx.x == 0) { dst[3 * R + 0] = v[0]; dst[3 * R + 1] = v[1]; }
}

// One workgroup, fp64, fixed order.  coef: [Rd][R][2] = (A, B) then one float bce_weight / (n_counted sum_r a_r)
// (Rd = batch_dice ? 1 : N); loss[3] = (L, L_dice, L_bce).
__global__ __launch_bounds__(256) void region_finalize_kernel(const float* __restrict__ part, const float* __restrict__ wdice,
                                                                const float* __restrict__ alpha_g, float* __restrict__ coef,
                                                                float* __restrict__ loss, int N, int R, int nblk, int batch_dice,
                                                                float dice_weight, float bce_weight) {
  __shared__ double red[8];
  double bce[2];   // the BCE numerator and the number of counted voxels
  compound_column_sum(bce, part + 3 * R, (i64)N * nblk, 3 * R + 2, red);
  const int Rd = batch_dice ? 1 : N;
  const double ldice = compound_region_finalize(part, wdice, coef, N, R, nblk, batch_dice, dice_weight, red);
  if (threadIdx.x == 0) {
    double asum = 0.0;
    for (int r = 0; r < R; ++r) asum += (double)alpha_g[r];
    const double den = bce[1] * asum;
    const double lb = den > 0.0 ? bce[0] / den : 0.0;
    double l = 0.0;
    if (dice_weight > 0.f) l += (double)dice_weight * ldice;
    if (bce_weight > 0.f) l += (double)bce_weight * lb;
    loss[0] = (float)l;
    loss[1] = (float)ldice;
    loss[2] = (float)lb;
    coef[2 * Rd * R] = (bce_weight > 0.f && den > 0.0) ? (float)((double)bce_weight / den) : 0.f;
  }
}

// grid compound_bwd_grid: the sample -- and with it the coefficient row -- is uniform per workgroup; all R planes of a voxel
// are read and written by the thread that owns it.
template <int CT, bool VEC>
__global__ __launch_bounds__(256) void region_bwd_kernel(const float* __restrict__ probs, const float* __restrict__ target,
                                                           RegionLut table, const float* __restrict__ coef,
                                                           const float* __restrict__ alpha_g, const float* __restrict__ gout,
                                                           float* __restrict__ dprobs, int R, i64 S, int Rd, float ignore,
                                                           float gamma) {
  constexpr int W = VEC ? 4 : 1;
  const unsigned* lut = table.stage();
  const int n = blockIdx.y;
  const float go = gout[0];
  const float cb = coef[2 * Rd * R];
  float A[CT], B[CT], alpha[CT];
  compound_load_coef<CT>(A, B, alpha, coef, Rd == 1 ? 0 : n, alpha_g, R);
  const float* tg = target + (i64)n * S;
  const float* pb = probs + (i64)n * R * S;
  float* db = dprobs + (i64)n * R * S;
  for (i64 s = ((i64)blockIdx.x * 256 + threadIdx.x) * W; s < S; s += (i64)gridDim.x * 256 * W) {
    float t[W];
    int bits[W];
    compound_load<W>(t, tg + s);
#pragma unroll
    for (int j = 0; j < W; ++j) bits[j] = region_bits(lut, t[j], ignore);
#pragma unroll
    for (int r = 0; r < CT; ++r)
      if (CT <= 5 || r < R) {
        float p[W], g[W];
        compound_load<W>(p, pb + (i64)r * S + s);
#pragma unroll
        for (int j = 0; j < W; ++j) {
          const bool z = (bits[j] >> r) & 1;
          const float q = z ? p[j] : 1.0f - p[j];
          float d = z ? A[r] + B[r] : B[r];
          if (cb != 0.f && q >= COMPOUND_PMIN) {
            const float dq = alpha[r] * cb * compound_dist_grad(q, gamma);
            d += z ? dq : -dq;
          }
          g[j] = bits[j] >= 0 ? go * d : 0.f;
        }
        compound_store<W>(db + (i64)r * S + s, g);
      }
  }
}

// ---- C ABI: the region loss (stands for no reference code; the stock-torch chain is a LUT gather, R masked sums and
// F.binary_cross_entropy) ----------------------------------------------------------------------------------------------------
extern "C" long long seg3d_region_loss_part_floats(int N, int R, long long S) {
  return (long long)N * seg3d_dice_blocks(S) * (3 * R + 2);
}

extern "C" int seg3d_region_loss_fwd(const float* probs, const float* target, const unsigned* lut_host, const float* wdice,
                                     const float* alpha, float* part, float* coef, float* loss, int N, int R, long long S,
                                     float gamma, float dice_weight, float bce_weight, int batch_dice, float ignore_label,
                                     void* stream) {
  SEG3D_REQUIRE(probs && target && lut_host && wdice && alpha && part && coef && loss && N > 0 && N <= 65535 && S > 0,
                "seg3d_region_loss_fwd: bad arguments");
  SEG3D_REQUIRE(R >= 1 && R <= SEG3D_MAXC, "seg3d_region_loss_fwd: %d regions not in [1, %d]", R, SEG3D_MAXC);
  SEG3D_REQUIRE(gamma >= 0.f && dice_weight >= 0.f && bce_weight >= 0.f && (dice_weight > 0.f || bce_weight > 0.f),
                "seg3d_region_loss_fwd: gamma and the term weights must be >= 0 and the weights not both 0");
  const int nblk = (int)seg3d_dice_blocks(S);
  const bool vec = compound_vec_ok(S, probs, target, probs);
  hipStream_t s = (hipStream_t)stream;
  const RegionLut table = region_table(lut_host);
  COMPOUND_DISPATCH(region_partial_kernel, R, vec,
                    <<<dim3(nblk, N), dim3(256), 0, s>>>(probs, target, table, alpha, part, R, (i64)S, nblk, ignore_label,
                                                         gamma));
  SEG3D_LAUNCH_CHECK("seg3d_region_loss_fwd(partial)");
  region_finalize_kernel<<<dim3(1), dim3(256), 0, s>>>(part, wdice, alpha, coef, loss, N, R, nblk, batch_dice ? 1 : 0,
                                                       dice_weight, bce_weight);
  SEG3D_LAUNCH_CHECK("seg3d_region_loss_fwd(finalize)");
  return SEG3D_OK;
}

extern "C" int seg3d_region_loss_bwd(const float* probs, const float* target, const unsigned* lut_host, const float* coef,
                                     const float* alpha, const float* gout, float* dprobs, int N, int R, long long S,
                                     float gamma, int batch_dice, float ignore_label, void* stream) {
  SEG3D_REQUIRE(probs && target && lut_host && coef && alpha && gout && dprobs && N > 0 && N <= 65535 && S > 0,
                "seg3d_region_loss_bwd: bad arguments");
  SEG3D_REQUIRE(R >= 1 && R <= SEG3D_MAXC, "seg3d_region_loss_bwd: %d regions not in [1, %d]", R, SEG3D_MAXC);
  SEG3D_REQUIRE(gamma >= 0.f, "seg3d_region_loss_bwd: gamma must be >= 0");
  const bool vec = compound_vec_ok(S, probs, target, dprobs);
  const int Rd = batch_dice ? 1 : N;
  const RegionLut table = region_table(lut_host);
  COMPOUND_DISPATCH(region_bwd_kernel, R, vec,
                    <<<compound_bwd_grid(S, N, vec), dim3(256), 0, (hipStream_t)stream>>>(probs, target, table, coef, alpha,
                                                                                         gout, dprobs, R, (i64)S, Rd,
                                                                                         ignore_label, gamma));
  SEG3D_LAUNCH_CHECK("seg3d_region_loss_bwd");
  return SEG3D_OK;
}
