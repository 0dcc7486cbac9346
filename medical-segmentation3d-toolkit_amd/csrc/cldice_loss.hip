// cldice_loss.hip -- soft-clDice topology loss (Shit et al., CVPR 2021) next to the compound loss's soft-Dice term, with
// the differentiable soft skeletons of the prediction and of the target computed on the device (no counterpart in the
// reference; definitions in DESIGN.md section 7, row f17, and include/seg3d_hip.h).
//   counted voxel:  the compound loss family's rule (compound_device.h); m(v) = 1 on counted voxels, 0 elsewhere
//   for sample n and class c of the class list K:  P_c = m p_c,  T_c = m [(int)t == c]
//   morphology (nothing exists outside the volume):
//     E(x)(v) = min of x over v and its 6 face neighbours inside the volume
//     D(x)(v) = max of x over the 3x3x3 neighbourhood inside the volume,   O(x) = D(E(x))
//   soft skeleton with k iterations:  x_0 = x,  s_0 = relu(x_0 - O(x_0));  for j = 1..k:  x_j = E(x_{j-1}),
//     d_j = relu(x_j - O(x_j)),  s_j = s_{j-1} + relu(d_j - s_{j-1} d_j);  skel_k(x) = s_k
//   SP = skel_k(P_c), ST = skel_k(T_c),  Tprec = (sum SP T_c + 1) / (sum SP + 1),  Tsens = (sum ST P_c + 1) / (sum ST + 1),
//   cl = 2 Tprec Tsens / (Tprec + Tsens),  L_cl = sum_{c in K} w'_c (1 - mean_n cl[n,c])   (batch_dice: the four sums are
//   summed over n first),  L = dice_weight L_dice + cldice_weight L_cl,  L_dice = the compound loss's soft-Dice term.
//
// One launch per stage j = 0..k (cld_stage_kernel): a workgroup stages its 32 x 8 x 8 tile of x_j with a halo of 2 in LDS
// (+inf outside the volume), computes E on the tile with a halo of 1 (-inf outside the volume), writes x_{j+1} for its
// own voxels, takes D from the staged E values (each thread walks a column of 8 voxels along z with the 3 x 3 maxima of
// its ten planes in registers) and updates the skeleton plane in place.  Stage 0 reads P_c or T_c straight from the
// probabilities / the target.
// Selection rule: a min or max that several positions attain sends its gradient to the position with the LOWEST LINEAR
// INDEX (z, then y, then x): the windows are walked in that order with a strict comparison.  relu' is 1 for a positive
// argument, 0 otherwise.
// What the backward needs of stage j is kept per voxel: one byte (bits 0..2: which of the 7 positions E took, bits 3..7:
// which of the 27 positions D took) and two floats, a_j = d s_j / d z_j (z_j = x_j - O(x_j)) and b_j = d s_j / d s_{j-1}.
// Backward, stage j = k..0 (cld_bwd_stage_kernel), in gather form: with gs = dL/ds_j staged as gz = gs a_j on the tile with
// a halo of 2, every voxel u of the tile with a halo of 1 collects  ge(u) = dL/dx_{j+1}(u) - sum gz(v)  over the
// neighbours v whose stored D selection points at u, then every tile voxel w collects  dL/dx_j(w) = gz(w) + sum ge(u)  over
// the neighbours u whose stored E selection points at w; dL/ds_{j-1} = gs b_j.  Fixed order, no atomics: bit-reproducible.
#include "seg3d_common.h"
#include "seg3d_hip.h"
#include "compound_device.h"

#define CLD_TX 32
#define CLD_TY 8
#define CLD_TZ 8
#define CLD_VOX (CLD_TX * CLD_TY * CLD_TZ)                      // 2048 voxels per workgroup, 8 per thread
#define CLD_H2X (CLD_TX + 4)
#define CLD_H2Y (CLD_TY + 4)
#define CLD_H2Z (CLD_TZ + 4)
#define CLD_H2 (CLD_H2X * CLD_H2Y * CLD_H2Z)                    // 5184
#define CLD_H1X (CLD_TX + 2)
#define CLD_H1Y (CLD_TY + 2)
#define CLD_H1Z (CLD_TZ + 2)
#define CLD_H1 (CLD_H1X * CLD_H1Y * CLD_H1Z)                    // 3400
#define CLD_MAX_AXIS 256
#define CLD_MAX_ITERS 16
#define CLD_INF __builtin_huge_valf()

enum { CLD_SRC_PLANE = 0, CLD_SRC_PROB = 1, CLD_SRC_TARGET = 2 };

struct CldGeom {
  int X, Y, Z, ntx, nty, K, C;
  float ignore;
  Seg3dClassList cls;
};

struct CldTile {
  int x0, y0, z0;
};
__device__ __forceinline__ CldTile cld_tile(const CldGeom& g) {
  const int b = blockIdx.x;
  CldTile t;
  t.x0 = (b % g.ntx) * CLD_TX;
  t.y0 = ((b / g.ntx) % g.nty) * CLD_TY;
  t.z0 = (b / (g.ntx * g.nty)) * CLD_TZ;
  return t;
}
__device__ __forceinline__ bool cld_inside(const CldGeom& g, int x, int y, int z) {
  return x >= 0 && x < g.X && y >= 0 && y < g.Y && z >= 0 && z < g.Z;
}

// voxel s of plane nk of the stage's input: a stored plane, P_c = m p_c or T_c = m [t == c]
template <int SRC>
__device__ __forceinline__ float cld_source(const float* __restrict__ plane, const float* __restrict__ probs,
                                            const float* __restrict__ target, const CldGeom& g, int nk, i64 S, i64 s) {
  if constexpr (SRC == CLD_SRC_PLANE) {
    return plane[(i64)nk * S + s];
  } else {
    const int n = nk / g.K, c = g.cls.id[nk % g.K];
    const int ci = compound_class(target[(i64)n * S + s], g.C, g.ignore);
    if constexpr (SRC == CLD_SRC_PROB) return ci >= 0 ? probs[((i64)n * g.C + c) * S + s] : 0.f;
    else return ci == c ? 1.f : 0.f;
  }
}

// A staged position of the tile with a halo of H: local and global coordinates, whether the voxel is inside the volume,
// and its linear index there (0 outside, so that a load from it is always legal and several can be in flight at once).
struct CldPos {
  int lx, ly, lz;
  bool in;
  i64 s;
};
template <int H>
__device__ __forceinline__ CldPos cld_pos(const CldGeom& g, const CldTile& t, int i) {
  constexpr int HX = CLD_TX + 2 * H, HY = CLD_TY + 2 * H, HZ = CLD_TZ + 2 * H;
  CldPos p;
  p.lx = i % HX;
  p.ly = (i / HX) % HY;
  p.lz = i / (HX * HY);
  const int x = t.x0 - H + p.lx, y = t.y0 - H + p.ly, z = t.z0 - H + p.lz;
  p.in = i < HX * HY * HZ && cld_inside(g, x, y, z);
  p.s = p.in ? ((i64)z * g.Y + y) * g.X + x : 0;
  return p;
}
#define CLD_BATCH 7   // independent global loads per thread before the first use: 3 x 7 x 256 >= CLD_H2, 2 x 7 x 256 >= CLD_H1

// One stage of the soft skeleton.  grid (tiles, planes), 256 threads.  xnext: x_{j+1} (null at the last stage); skel: s_j,
// updated in place (FIRST: written).  SAVE: sa / sb / sel of this stage for the backward.
// Thread (lx, ly) = (tid % 32, tid / 32) owns the tile's column of 8 voxels along z: the 3 x 3 plane maxima of its ten
// staged planes are taken once each, and D of a voxel is the first largest of three of them.
template <int SRC, bool FIRST, bool SAVE>
__global__ __launch_bounds__(256) void cld_stage_kernel(const float* __restrict__ plane, const float* __restrict__ probs,
                                                          const float* __restrict__ target, float* __restrict__ xnext,
                                                          float* __restrict__ skel, float* __restrict__ sa,
                                                          float* __restrict__ sb, unsigned char* __restrict__ sel,
                                                          CldGeom g) {
  __shared__ float xs[CLD_H2];
  __shared__ float es[CLD_H1];
  __shared__ unsigned char se[CLD_VOX];
  const CldTile t = cld_tile(g);
  const int nk = blockIdx.y;
  const i64 S = (i64)g.X * g.Y * g.Z;
  for (int i0 = threadIdx.x; i0 < CLD_H2; i0 += 256 * CLD_BATCH) {
    float v[CLD_BATCH];
#pragma unroll
    for (int u = 0; u < CLD_BATCH; ++u) {
      const CldPos p = cld_pos<2>(g, t, i0 + 256 * u);
      v[u] = cld_source<SRC>(plane, probs, target, g, nk, S, p.s);
      if (!p.in) v[u] = CLD_INF;
    }
#pragma unroll
    for (int u = 0; u < CLD_BATCH; ++u)
      if (i0 + 256 * u < CLD_H2) xs[i0 + 256 * u] = v[u];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < CLD_H1; i += 256) {
    const CldPos p = cld_pos<1>(g, t, i);
    const int c = ((p.lz + 1) * CLD_H2Y + (p.ly + 1)) * CLD_H2X + (p.lx + 1);
    const int off[7] = {-CLD_H2X * CLD_H2Y, -CLD_H2X, -1, 0, 1, CLD_H2X, CLD_H2X * CLD_H2Y};   // lowest linear index first
    float e = xs[c + off[0]];
    int code = 0;
#pragma unroll
    for (int q = 1; q < 7; ++q) {
      const float v = xs[c + off[q]];
      if (v < e) {
        e = v;
        code = q;
      }
    }
    es[i] = p.in ? e : -CLD_INF;
    const bool own = p.in && p.lx >= 1 && p.lx <= CLD_TX && p.ly >= 1 && p.ly <= CLD_TY && p.lz >= 1 && p.lz <= CLD_TZ;
    if (own) {
      se[((p.lz - 1) * CLD_TY + (p.ly - 1)) * CLD_TX + (p.lx - 1)] = (unsigned char)code;
      if (xnext) xnext[(i64)nk * S + p.s] = e;
    }
  }
  __syncthreads();
  const int lx = threadIdx.x % CLD_TX, ly = threadIdx.x / CLD_TX;
  const int x = t.x0 + lx, y = t.y0 + ly;
  if (x >= g.X || y >= g.Y) return;
  float pm[CLD_H1Z];   // the first largest of the 3 x 3 window of plane pz around (lx, ly), and which of the 9 it is
  int pc[CLD_H1Z];
#pragma unroll
  for (int pz = 0; pz < CLD_H1Z; ++pz) {
    const int c = (pz * CLD_H1Y + (ly + 1)) * CLD_H1X + (lx + 1);
    pm[pz] = -CLD_INF;
    pc[pz] = 4;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const float v = es[c + dy * CLD_H1X + dx];
        if (v > pm[pz]) {
          pm[pz] = v;
          pc[pz] = (dy + 1) * 3 + (dx + 1);
        }
      }
  }
#pragma unroll
  for (int lz = 0; lz < CLD_TZ; ++lz) {
    const int z = t.z0 + lz;
    if (z >= g.Z) continue;
    float o = pm[lz];
    int code = pc[lz];
    if (pm[lz + 1] > o) {
      o = pm[lz + 1];
      code = 9 + pc[lz + 1];
    }
    if (pm[lz + 2] > o) {
      o = pm[lz + 2];
      code = 18 + pc[lz + 2];
    }
    const float xc = xs[((lz + 2) * CLD_H2Y + (ly + 2)) * CLD_H2X + (lx + 2)];
    const float d = fmaxf(xc - o, 0.f);
    const i64 gi = (i64)nk * S + ((i64)z * g.Y + y) * g.X + x;
    float s, a, b;
    if constexpr (FIRST) {
      s = d;
      a = d > 0.f ? 1.f : 0.f;
      b = 0.f;
    } else {
      const float sp = skel[gi];
      const float u = d - sp * d;
      s = sp + fmaxf(u, 0.f);
      a = u > 0.f ? 1.f - sp : 0.f;
      b = u > 0.f ? 1.f - d : 1.f;
    }
    skel[gi] = s;
    if constexpr (SAVE) {
      sa[gi] = a;
      sb[gi] = b;
      sel[gi] = (unsigned char)(se[(lz * CLD_TY + ly) * CLD_TX + lx] | (code << 3));
    }
  }
}

// One stage of the backward.  grid (tiles, planes), 256 threads.  LAST (stage k): dL/ds_k = a1 T_c + a2 from the
// coefficient row of (r, k) and there is no dL/dx_{k+1}; otherwise gs_in / gxn.  STAGE0: no dL/ds_{-1} is written.
template <bool LAST, bool STAGE0>
__global__ __launch_bounds__(256) void cld_bwd_stage_kernel(const float* __restrict__ gs_in, float* __restrict__ gs_out,
                                                              const float* __restrict__ gxn, float* __restrict__ gx_out,
                                                              const float* __restrict__ sa, const float* __restrict__ sb,
                                                              const unsigned char* __restrict__ sel,
                                                              const float* __restrict__ target,
                                                              const float* __restrict__ ccoef, int R, CldGeom g) {
  __shared__ float gz[CLD_H2];
  __shared__ float ge[CLD_H1];
  __shared__ unsigned char sl[CLD_H2];
  const CldTile t = cld_tile(g);
  const int nk = blockIdx.y;
  const i64 S = (i64)g.X * g.Y * g.Z;
  const int n = nk / g.K, k = nk % g.K;
  float a1 = 0.f, a2 = 0.f;
  if constexpr (LAST) {
    const float* row = ccoef + 3 * ((R == 1 ? 0 : n) * g.K + k);
    a1 = row[0];
    a2 = row[1];
  }
  // dL/ds_j of voxel s of this plane
  auto grad_s = [&](i64 s) -> float {
    if constexpr (LAST) return compound_class(target[(i64)n * S + s], g.C, g.ignore) == g.cls.id[k] ? a1 + a2 : a2;
    else return gs_in[(i64)nk * S + s];
  };
  for (int i0 = threadIdx.x; i0 < CLD_H2; i0 += 256 * CLD_BATCH) {
    float v[CLD_BATCH];
    unsigned char sv[CLD_BATCH];
#pragma unroll
    for (int u = 0; u < CLD_BATCH; ++u) {
      const CldPos p = cld_pos<2>(g, t, i0 + 256 * u);
      v[u] = grad_s(p.s) * sa[(i64)nk * S + p.s];
      sv[u] = sel[(i64)nk * S + p.s];
      if (!p.in) {
        v[u] = 0.f;
        sv[u] = 0xff;   // points at nothing
      }
    }
#pragma unroll
    for (int u = 0; u < CLD_BATCH; ++u)
      if (i0 + 256 * u < CLD_H2) {
        gz[i0 + 256 * u] = v[u];
        sl[i0 + 256 * u] = sv[u];
      }
  }
  __syncthreads();
  for (int i0 = threadIdx.x; i0 < CLD_H1; i0 += 256 * CLD_BATCH) {
    float acc[CLD_BATCH];
#pragma unroll
    for (int u = 0; u < CLD_BATCH; ++u) {
      acc[u] = 0.f;
      if constexpr (!LAST) {
        const CldPos p = cld_pos<1>(g, t, i0 + 256 * u);
        acc[u] = gxn[(i64)nk * S + p.s];
        if (!p.in) acc[u] = 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < CLD_BATCH; ++u) {
      const int i = i0 + 256 * u;
      if (i >= CLD_H1) continue;
      const CldPos p = cld_pos<1>(g, t, i);
      if (p.in) {
        const int c = ((p.lz + 1) * CLD_H2Y + (p.ly + 1)) * CLD_H2X + (p.lx + 1);
#pragma unroll
        for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
          for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
              const int v = c + (dz * CLD_H2Y + dy) * CLD_H2X + dx;
              // the neighbour at +delta took position -delta of its own window: it took this voxel
              const int want = 26 - ((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1));
              const float gv = gz[v];   // read unconditionally: no branch per neighbour, the reads pipeline
              acc[u] -= (sl[v] >> 3) == want ? gv : 0.f;
            }
      }
      ge[i] = acc[u];
    }
  }
  __syncthreads();
  const int lx = threadIdx.x % CLD_TX, ly = threadIdx.x / CLD_TX;
  const int x = t.x0 + lx, y = t.y0 + ly;
  if (x >= g.X || y >= g.Y) return;
#pragma unroll
  for (int lz = 0; lz < CLD_TZ; ++lz) {
    const int z = t.z0 + lz;
    if (z >= g.Z) continue;
    const i64 s = ((i64)z * g.Y + y) * g.X + x;
    const int c2 = ((lz + 2) * CLD_H2Y + (ly + 2)) * CLD_H2X + (lx + 2);
    const int c1 = ((lz + 1) * CLD_H1Y + (ly + 1)) * CLD_H1X + (lx + 1);
    const int off2[7] = {-CLD_H2X * CLD_H2Y, -CLD_H2X, -1, 0, 1, CLD_H2X, CLD_H2X * CLD_H2Y};
    const int off1[7] = {-CLD_H1X * CLD_H1Y, -CLD_H1X, -1, 0, 1, CLD_H1X, CLD_H1X * CLD_H1Y};
    float acc = gz[c2];
#pragma unroll
    for (int p = 0; p < 7; ++p) {
      const float ev = ge[c1 + off1[p]];
      acc += (sl[c2 + off2[p]] & 7) == 6 - p ? ev : 0.f;
    }
    gx_out[(i64)nk * S + s] = acc;
    if constexpr (!STAGE0) gs_out[(i64)nk * S + s] = grad_s(s) * sb[(i64)nk * S + s];
  }
}

// ---- the loss ----------------------------------------------------------------------------------------------------------
// the compound loss's region partial sums (its walk, its voxel rule, its store): part[n][blk][3C + 2], last two slots 0
template <int CT, bool VEC>
__global__ __launch_bounds__(256) void cld_region_partial_kernel(const float* __restrict__ probs,
                                                                   const float* __restrict__ target, float* __restrict__ part,
                                                                   int C, i64 S, int nblk, float ignore) {
  constexpr int W = VEC ? 4 : 1;
  __shared__ float red[4 * 3];
  float zero[CT] = {};
  CompoundAcc<CT> a;
  compound_block_walk<CT, W>(probs, target, C, S, [&](i64, const float (&t)[W], const float (&p)[W][CT]) {
#pragma unroll
    for (int j = 0; j < W; ++j) {
      float pt, at;
      compound_region_voxel<CT>(a, t[j], p[j], zero, C, ignore, pt, at);
    }
  });
  float* dst = compound_region_store<CT>(a, part, C, nblk, red);
  if (threadIdx.x == 0) {
    dst[3 * C + 0] = 0.f;
    dst[3 * C + 1] = 0.f;
  }
}

// cpart[k][n][blk][4] = (sum SP T_c, sum SP, sum ST P_c, sum ST) over the block's DICE_VPB voxels.  grid (nblk, N * K)
__global__ __launch_bounds__(256) void cld_sums_kernel(const float* __restrict__ probs, const float* __restrict__ target,
                                                         const float* __restrict__ sp, const float* __restrict__ st,
                                                         float* __restrict__ cpart, int N, i64 S, int nblk, CldGeom g) {
  __shared__ float red[4 * 4];
  const int nk = blockIdx.y, n = nk / g.K, k = nk % g.K, c = g.cls.id[k];
  const i64 s0 = (i64)blockIdx.x * DICE_VPB;
  i64 s1 = s0 + DICE_VPB;
  if (s1 > S) s1 = S;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  for (i64 s = s0 + threadIdx.x; s < s1; s += 256) {
    const int ci = compound_class(target[(i64)n * S + s], g.C, g.ignore);
    const float p = ci >= 0 ? probs[((i64)n * g.C + c) * S + s] : 0.f;
    const float a = sp[(i64)nk * S + s], b = st[(i64)nk * S + s];
    v[0] += ci == c ? a : 0.f;
    v[1] += a;
    v[2] = fmaf(b, p, v[2]);
    v[3] += b;
  }
  block_sum_256<4>(v, red);
  if (threadIdx.x == 0) {
    float* dst = cpart + (((i64)k * N + n) * nblk + blockIdx.x) * 4;
    dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2]; dst[3] = v[3];
  }
}

// One workgroup, fp64, fixed order.  coef: [R][C][2] = (A, B) of the region term, then ccoef[R][K][3] = (a1, a2, a3):
//   dL/dSP(v) = a1 T_c(v) + a2,  dL/dP_c(v) = a3 ST(v)  (the part that does not pass through the skeleton)
__global__ __launch_bounds__(256) void cld_finalize_kernel(const float* __restrict__ part, const float* __restrict__ cpart,
                                                             const float* __restrict__ wdice, const float* __restrict__ wcl,
                                                             float* __restrict__ coef, float* __restrict__ loss, int N, int C,
                                                             int K, int nblk, int batch_dice, float dice_weight,
                                                             float cldice_weight) {
  __shared__ double red[16];
  __shared__ double lsum;
  const int R = batch_dice ? 1 : N;
  const double lr = compound_region_finalize(part, wdice, coef, N, C, nblk, batch_dice, dice_weight, red);
  __syncthreads();
  if (threadIdx.x == 0) lsum = 0.0;
  float* ccoef = coef + 2 * R * C;
  for (int k = 0; k < K; ++k)
    for (int r = 0; r < R; ++r) {
      double v[4];
      compound_column_sum(v, cpart + ((i64)k * N + r) * nblk * 4, batch_dice ? (i64)N * nblk : (i64)nblk, 4, red);
      if (threadIdx.x == 0) {
        const double w = (double)wcl[k];
        const double tp = (v[0] + 1.0) / (v[1] + 1.0), ts = (v[2] + 1.0) / (v[3] + 1.0);
        const double cl = 2.0 * tp * ts / (tp + ts);
        lsum += w * (1.0 - cl) / (double)R;
        const double q = -(double)cldice_weight * w / (double)R;        // dL / dcl
        const double dtp = q * 2.0 * ts * ts / ((tp + ts) * (tp + ts));  // dL / dTprec
        const double dts = q * 2.0 * tp * tp / ((tp + ts) * (tp + ts));  // dL / dTsens
        float* row = ccoef + 3 * (r * K + k);
        row[0] = (float)(dtp / (v[1] + 1.0));
        row[1] = (float)(-dtp * (v[0] + 1.0) / ((v[1] + 1.0) * (v[1] + 1.0)));
        row[2] = (float)(dts / (v[3] + 1.0));
      }
    }
  if (threadIdx.x == 0) {
    const double lc = lsum;
    double l = 0.0;
    if (dice_weight > 0.f) l += (double)dice_weight * lr;
    if (cldice_weight > 0.f) l += (double)cldice_weight * lc;
    loss[0] = (float)l;
    loss[1] = (float)lr;
    loss[2] = (float)lc;
  }
}

// grid (blocks, N); all C planes in one pass.  gx0: dL/dP_c through the skeleton, [N][K][S] (null: no clDice part)
template <int CT, bool VEC>
__global__ __launch_bounds__(256) void cld_bwd_kernel(const float* __restrict__ target, const float* __restrict__ gx0,
                                                        const float* __restrict__ st, const float* __restrict__ coef,
                                                        const float* __restrict__ gout, float* __restrict__ dprobs, int C,
                                                        i64 S, int R, int K, Seg3dClassList cls, float ignore) {
  constexpr int W = VEC ? 4 : 1;
  const int n = blockIdx.y;
  const float go = gout[0];
  float A[CT], B[CT], a3[CT];
  int kof[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    const bool on = CT <= 5 || c < C;
    A[c] = on ? coef[2 * ((R == 1 ? 0 : n) * C + c) + 0] : 0.f;
    B[c] = on ? coef[2 * ((R == 1 ? 0 : n) * C + c) + 1] : 0.f;
    kof[c] = -1;
    a3[c] = 0.f;
  }
  if (gx0) {
    const float* ccoef = coef + 2 * R * C + 3 * (R == 1 ? 0 : n) * K;
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int c = 0; c < CT; ++c)
        if (cls.id[k] == c) {
          kof[c] = k;
          a3[c] = ccoef[3 * k + 2];
        }
  }
  const float* tg = target + (i64)n * S;
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
        float x[W] = {}, y[W] = {}, gr[W];
        if (kof[c] >= 0) {
          compound_load<W>(x, gx0 + ((i64)n * K + kof[c]) * S + s);
          compound_load<W>(y, st + ((i64)n * K + kof[c]) * S + s);
        }
#pragma unroll
        for (int j = 0; j < W; ++j)
          gr[j] = ti[j] >= 0 ? go * ((ti[j] == c ? A[c] + B[c] : B[c]) + fmaf(a3[c], y[j], x[j])) : 0.f;
        compound_store<W>(db + (i64)c * S + s, gr);
      }
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
static int cld_geom(CldGeom& g, int X, int Y, int Z, int K, int C, float ignore, const Seg3dClassList* cls) {
  g.X = X; g.Y = Y; g.Z = Z;
  g.ntx = (X + CLD_TX - 1) / CLD_TX;
  g.nty = (Y + CLD_TY - 1) / CLD_TY;
  g.K = K; g.C = C; g.ignore = ignore;
  for (int i = 0; i < 16; ++i) g.cls.id[i] = cls ? cls->id[i] : 0;
  return g.ntx * g.nty * ((Z + CLD_TZ - 1) / CLD_TZ);
}

// the k + 1 stages of one skeleton: stage 0 reads SRC, stage j >= 1 the plane the stage before wrote (xa / xb in turns)
template <int SRC, bool SAVE>
static void cld_skeleton(const float* plane, const float* probs, const float* target, float* skel, float* xa, float* xb,
                         float* sa, float* sb, unsigned char* sel, i64 stage_stride, int planes, int iters, const CldGeom& g,
                         int tiles, hipStream_t s) {
  const dim3 grid(tiles, planes);
  cld_stage_kernel<SRC, true, SAVE><<<grid, dim3(256), 0, s>>>(plane, probs, target, xa, skel, sa, sb, sel, g);
  for (int j = 1; j <= iters; ++j) {
    const float* cur = (j & 1) ? xa : xb;
    float* next = j == iters ? nullptr : ((j & 1) ? xb : xa);
    cld_stage_kernel<CLD_SRC_PLANE, false, SAVE><<<grid, dim3(256), 0, s>>>(
        cur, probs, target, next, skel, SAVE ? sa + j * stage_stride : sa, SAVE ? sb + j * stage_stride : sb,
        SAVE ? sel + j * stage_stride : sel, g);
  }
}

static bool cld_shape_ok(int X, int Y, int Z, int iters) {
  return X >= 1 && X <= CLD_MAX_AXIS && Y >= 1 && Y <= CLD_MAX_AXIS && Z >= 1 && Z <= CLD_MAX_AXIS && iters >= 1 &&
         iters <= CLD_MAX_ITERS;
}

extern "C" long long seg3d_soft_skeleton_workspace_bytes(long long planes, int X, int Y, int Z) {
  if (planes <= 0 || X <= 0 || Y <= 0 || Z <= 0) return 0;
  return 2 * planes * X * Y * Z * 4;
}

extern "C" int seg3d_soft_skeleton(const float* x, float* skel, void* workspace, long long planes, int X, int Y, int Z,
                                   int iters, void* stream) {
  SEG3D_REQUIRE(x && skel && x != skel && workspace && planes > 0 && planes <= 65535, "seg3d_soft_skeleton: bad arguments");
  SEG3D_REQUIRE(cld_shape_ok(X, Y, Z, iters), "seg3d_soft_skeleton: axes (%d, %d, %d) not in [1, %d] or iters %d not in [1, %d]",
                X, Y, Z, CLD_MAX_AXIS, iters, CLD_MAX_ITERS);
  const i64 S = (i64)X * Y * Z;
  SEG3D_REQUIRE(planes * S < (1ll << 31), "seg3d_soft_skeleton: planes * S = %lld not below 2^31", planes * S);
  CldGeom g;
  const int tiles = cld_geom(g, X, Y, Z, 1, 1, -1.f, nullptr);
  float* xa = reinterpret_cast<float*>(workspace);
  cld_skeleton<CLD_SRC_PLANE, false>(x, nullptr, nullptr, skel, xa, xa + planes * S, nullptr, nullptr, nullptr, 0, (int)planes,
                                     iters, g, tiles, (hipStream_t)stream);
  SEG3D_LAUNCH_CHECK("seg3d_soft_skeleton");
  return SEG3D_OK;
}

// workspace, in floats (every offset a multiple of 4): Dice partial sums | clDice partial sums | SP | ST | four planes
// (x_j in turns forward; dL/ds and dL/dx in turns backward) | a_j | b_j (k + 1 stages each) | selection bytes
struct CldLayout {
  i64 cpart, sp, st, buf, sa, sb, sel, total_bytes;
};
static CldLayout cld_layout(int N, int C, int K, i64 S, int iters) {
  auto up4 = [](i64 v) { return (v + 3) & ~(i64)3; };
  const i64 P = up4((i64)N * K * S);
  CldLayout l;
  l.cpart = up4(seg3d_compound_loss_part_floats(N, C, S));
  l.sp = l.cpart + up4((i64)K * N * seg3d_dice_blocks(S) * 4);
  l.st = l.sp + P;
  l.buf = l.st + P;
  l.sa = l.buf + 4 * P;
  l.sb = l.sa + (iters + 1) * P;
  l.sel = l.sb + (iters + 1) * P;
  l.total_bytes = l.sel * 4 + up4((iters + 1) * P);
  return l;
}

static int cld_loss_args(const char* who, int N, int C, int X, int Y, int Z, const Seg3dClassList& cls, int K, int iters) {
  SEG3D_REQUIRE(N > 0, "%s: bad arguments", who);
  SEG3D_REQUIRE(C >= 1 && C <= SEG3D_MAXC, "%s: num_class %d not in [1, %d]", who, C, SEG3D_MAXC);
  SEG3D_REQUIRE(cld_shape_ok(X, Y, Z, iters), "%s: axes (%d, %d, %d) not in [1, %d] or iters %d not in [1, %d]", who, X, Y, Z,
                CLD_MAX_AXIS, iters, CLD_MAX_ITERS);
  SEG3D_REQUIRE(K >= 1 && K <= SEG3D_MAXC, "%s: %d class ids, not in [1, %d]", who, K, SEG3D_MAXC);
  for (int k = 0; k < K; ++k) {
    SEG3D_REQUIRE(cls.id[k] >= 0 && cls.id[k] < C, "%s: class id %d not in [0, %d)", who, cls.id[k], C);
    for (int q = 0; q < k; ++q) SEG3D_REQUIRE(cls.id[q] != cls.id[k], "%s: class id %d listed twice", who, cls.id[k]);
  }
  SEG3D_REQUIRE((i64)N * K <= 65535, "%s: N * K = %lld above 65535", who, (i64)N * K);
  SEG3D_REQUIRE((i64)N * X * Y * Z < (1ll << 31), "%s: N * S = %lld not below 2^31", who, (i64)N * X * Y * Z);
  return SEG3D_OK;
}

extern "C" long long seg3d_cldice_loss_workspace_bytes(int N, int C, int K, int X, int Y, int Z, int iters) {
  if (N <= 0 || C <= 0 || K <= 0 || X <= 0 || Y <= 0 || Z <= 0 || iters <= 0) return 0;
  return cld_layout(N, C, K, (i64)X * Y * Z, iters).total_bytes;
}

extern "C" int seg3d_cldice_loss_fwd(const float* probs, const float* target, const float* wdice, const float* wcl,
                                     void* workspace, float* coef, float* loss, int N, int C, int X, int Y, int Z,
                                     Seg3dClassList class_ids, int K, int iters, float dice_weight, float cldice_weight,
                                     int batch_dice, float ignore_label, void* stream) {
  SEG3D_REQUIRE(probs && target && wdice && wcl && workspace && coef && loss, "seg3d_cldice_loss_fwd: bad arguments");
  if (int e = cld_loss_args("seg3d_cldice_loss_fwd", N, C, X, Y, Z, class_ids, K, iters)) return e;
  SEG3D_REQUIRE(dice_weight >= 0.f && cldice_weight >= 0.f && (dice_weight > 0.f || cldice_weight > 0.f),
                "seg3d_cldice_loss_fwd: the term weights must be >= 0 and not both 0");
  SEG3D_REQUIRE(((uintptr_t)workspace & 15) == 0, "seg3d_cldice_loss_fwd: the workspace must be 16-byte aligned");
  const i64 S = (i64)X * Y * Z;
  const int nblk = (int)seg3d_dice_blocks(S);
  const CldLayout l = cld_layout(N, C, K, S, iters);
  const i64 P = (l.st - l.sp);
  float* ws = reinterpret_cast<float*>(workspace);
  float *part = ws, *cpart = ws + l.cpart, *sp = ws + l.sp, *st = ws + l.st, *xa = ws + l.buf, *xb = xa + P;
  hipStream_t s = (hipStream_t)stream;
  const bool vec = compound_vec_ok(S, probs, target, probs);   // the compound loss's own choice: same order of additions
  COMPOUND_DISPATCH(cld_region_partial_kernel, C, vec,
                    <<<dim3(nblk, N), dim3(256), 0, s>>>(probs, target, part, C, S, nblk, ignore_label));
  SEG3D_LAUNCH_CHECK("seg3d_cldice_loss_fwd(region)");
  CldGeom g;
  const int tiles = cld_geom(g, X, Y, Z, K, C, ignore_label, &class_ids);
  cld_skeleton<CLD_SRC_TARGET, false>(nullptr, probs, target, st, xa, xb, nullptr, nullptr, nullptr, 0, N * K, iters, g, tiles, s);
  SEG3D_LAUNCH_CHECK("seg3d_cldice_loss_fwd(target skeleton)");
  unsigned char* sel = reinterpret_cast<unsigned char*>(ws + l.sel);
  if (cldice_weight > 0.f)
    cld_skeleton<CLD_SRC_PROB, true>(nullptr, probs, target, sp, xa, xb, ws + l.sa, ws + l.sb, sel, P, N * K, iters, g, tiles, s);
  else   // the term is reported but has no backward: nothing is kept
    cld_skeleton<CLD_SRC_PROB, false>(nullptr, probs, target, sp, xa, xb, nullptr, nullptr, nullptr, 0, N * K, iters, g, tiles, s);
  SEG3D_LAUNCH_CHECK("seg3d_cldice_loss_fwd(prediction skeleton)");
  cld_sums_kernel<<<dim3(nblk, N * K), dim3(256), 0, s>>>(probs, target, sp, st, cpart, N, S, nblk, g);
  SEG3D_LAUNCH_CHECK("seg3d_cldice_loss_fwd(sums)");
  cld_finalize_kernel<<<dim3(1), dim3(256), 0, s>>>(part, cpart, wdice, wcl, coef, loss, N, C, K, nblk, batch_dice ? 1 : 0,
                                                    dice_weight, cldice_weight);
  SEG3D_LAUNCH_CHECK("seg3d_cldice_loss_fwd(finalize)");
  return SEG3D_OK;
}

extern "C" int seg3d_cldice_loss_bwd(const float* target, void* workspace, const float* coef, const float* gout, float* dprobs,
                                     int N, int C, int X, int Y, int Z, Seg3dClassList class_ids, int K, int iters,
                                     float cldice_weight, int batch_dice, float ignore_label, void* stream) {
  SEG3D_REQUIRE(target && workspace && coef && gout && dprobs, "seg3d_cldice_loss_bwd: bad arguments");
  if (int e = cld_loss_args("seg3d_cldice_loss_bwd", N, C, X, Y, Z, class_ids, K, iters)) return e;
  SEG3D_REQUIRE(cldice_weight >= 0.f, "seg3d_cldice_loss_bwd: cldice_weight must be >= 0");
  SEG3D_REQUIRE(((uintptr_t)workspace & 15) == 0, "seg3d_cldice_loss_bwd: the workspace must be 16-byte aligned");
  const i64 S = (i64)X * Y * Z;
  const CldLayout l = cld_layout(N, C, K, S, iters);
  const i64 P = (l.st - l.sp);
  float* ws = reinterpret_cast<float*>(workspace);
  const float *st = ws + l.st, *sa = ws + l.sa, *sb = ws + l.sb;
  const unsigned char* sel = reinterpret_cast<const unsigned char*>(ws + l.sel);
  float* gs[2] = {ws + l.buf, ws + l.buf + P};
  float* gx[2] = {ws + l.buf + 2 * P, ws + l.buf + 3 * P};
  hipStream_t s = (hipStream_t)stream;
  const int R = batch_dice ? 1 : N;
  const float* ccoef = coef + 2 * R * C;
  const float* gx0 = nullptr;
  if (cldice_weight > 0.f) {
    CldGeom g;
    const int tiles = cld_geom(g, X, Y, Z, K, C, ignore_label, &class_ids);
    const dim3 grid(tiles, N * K);
    // stage j reads dL/ds_j from gs[j & 1] and dL/dx_{j+1} from gx[(j + 1) & 1], writes gs[(j - 1) & 1] and gx[j & 1]
    cld_bwd_stage_kernel<true, false><<<grid, dim3(256), 0, s>>>(nullptr, gs[(iters - 1) & 1], nullptr, gx[iters & 1],
                                                                 sa + iters * P, sb + iters * P, sel + iters * P, target, ccoef,
                                                                 R, g);
    for (int j = iters - 1; j >= 1; --j)
      cld_bwd_stage_kernel<false, false><<<grid, dim3(256), 0, s>>>(gs[j & 1], gs[(j - 1) & 1], gx[(j + 1) & 1], gx[j & 1],
                                                                    sa + j * P, sb + j * P, sel + j * P, target, ccoef, R, g);
    cld_bwd_stage_kernel<false, true><<<grid, dim3(256), 0, s>>>(gs[0], nullptr, gx[1], gx[0], sa, sb, sel, target, ccoef, R, g);
    SEG3D_LAUNCH_CHECK("seg3d_cldice_loss_bwd(skeleton)");
    gx0 = gx[0];
  }
  const bool vec = compound_vec_ok(S, target, ws, dprobs);
  COMPOUND_DISPATCH(cld_bwd_kernel, C, vec,
                    <<<compound_bwd_grid(S, N, vec), dim3(256), 0, s>>>(target, gx0, st, coef, gout, dprobs, C, S, R, K,
                                                                        class_ids, ignore_label));
  SEG3D_LAUNCH_CHECK("seg3d_cldice_loss_bwd");
  return SEG3D_OK;
}
