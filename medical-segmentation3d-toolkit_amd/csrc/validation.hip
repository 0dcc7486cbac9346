// validation.hip -- arg-max + per-class confusion counts of a probability map against a label map, for the validation pass
// that runs between training epochs.
//
// Replaces nothing in the reference: its core/seg_train.py never measures the model while it trains.  The stock-torch chain
// this stands for is `pred = probs.argmax(1)` followed by 3 C masked sums (C + 1 reads of the label-sized tensors each).
// Here ONE streaming pass over probs [N][C][S] (planar fp32, what the soft-max head writes) and target [N][S] (float class
// ids, what the losses take) adds, for every valid voxel,
//     tp[c] += [pred == c && t == c]      fp[c] += [pred == c && t != c]      fn[c] += [pred != c && t == c]
// into counts[c] = (tp, fp, fn).  valid is the compound loss's rule (compound_device.h compound_class): t >= 0 && t < C &&
// t != ignore, class (int)t.  pred is the FIRST maximum: class 0, replaced only by a strictly greater value (finalize_argmax_kernel,
// tensor.max(0)).  NaN probabilities are outside the contract: every comparison with a NaN is false, so a NaN in a class
// above 0 never becomes the maximum and a NaN in class 0 is never replaced (np.argmax would return the NaN's index in both
// cases).  Integer counting only: per-thread 32-bit counters, a wave64
// shuffle sum, one LDS row per wave, then 3 C 64-bit integer atomics per workgroup -- bit-exact in any order.
// HBM-bound: algorithmic bytes = (C + 1) * 4 per voxel.
#include "seg3d_common.h"
#include "seg3d_hip.h"
#include "compound_device.h"   // SEG3D_MAXC, compound_class, compound_load
#include "region_device.h"     // RegionLut, region_bits: the table and the counting rule of region-based models

#define CONF_THREADS 1024
#define CONF_WAVES (CONF_THREADS / 64)

// CT = C for C <= 5 (fully unrolled, no guards); CT = 16 serves 6..16 classes with `c < C` guards, as in loss.hip
template <int CT>
struct ConfAcc {
  unsigned tp[CT], fp[CT], fn[CT];
};

template <int CT>
__device__ __forceinline__ void conf_voxel(ConfAcc<CT>& a, float t, int pred, int C, float ignore) {
  const int ti = compound_class(t, C, ignore);
  if (ti < 0) return;
#pragma unroll
  for (int c = 0; c < CT; ++c)
    if (CT <= 5 || c < C) {
      const bool p = pred == c, g = ti == c;
      a.tp[c] += (p && g) ? 1u : 0u;
      a.fp[c] += (p && !g) ? 1u : 0u;
      a.fn[c] += (!p && g) ? 1u : 0u;
    }
}

// The workgroup's counters into counts[3 * C]: a wave64 shuffle sum, one LDS row per wave, then at most 3 C 64-bit integer
// atomics.  Every thread calls it once, after its walk.  A thread counts at most S / 1024 + 4 voxels and a wave 64 times that:
// 32 bits hold both for S < 2^33 (checked by the entries).
template <int CT>
__device__ __forceinline__ void conf_commit(const ConfAcc<CT>& a, int C, unsigned long long* __restrict__ counts) {
  __shared__ unsigned red[CONF_WAVES][3 * CT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < CT; ++c)
    if (CT <= 5 || c < C) {
      unsigned x = a.tp[c], y = a.fp[c], z = a.fn[c];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        x += __shfl_down(x, off, 64);
        y += __shfl_down(y, off, 64);
        z += __shfl_down(z, off, 64);
      }
      if (lane == 0) {
        red[wave][3 * c + 0] = x;
        red[wave][3 * c + 1] = y;
        red[wave][3 * c + 2] = z;
      }
    }
  __syncthreads();
  if ((int)threadIdx.x < 3 * C) {
    unsigned long long v = 0ull;
#pragma unroll
    for (int w = 0; w < CONF_WAVES; ++w) v += red[w][threadIdx.x];
    if (v) atomicAdd(counts + threadIdx.x, v);   // integer atomics: the result does not depend on the order
  }
}

// grid (gx, N): workgroup (bx, n) strides over sample n's voxels.  counts: 3 * C u64, ADDED to.
template <int CT, bool VEC>
__global__ __launch_bounds__(CONF_THREADS) void confusion_counts_kernel(const float* __restrict__ probs,
                                                                         const float* __restrict__ target,
                                                                         unsigned long long* __restrict__ counts, int C, i64 S,
                                                                         float ignore) {
  const int n = blockIdx.y;
  const float* tg = target + (i64)n * S;
  const float* pb = probs + (i64)n * C * S;
  ConfAcc<CT> a;
#pragma unroll
  for (int c = 0; c < CT; ++c) a.tp[c] = a.fp[c] = a.fn[c] = 0u;
  constexpr int W = VEC ? 4 : 1;   // VEC: S % 4 == 0 and 16-byte aligned bases, so every plane row starts aligned
  for (i64 s = ((i64)blockIdx.x * CONF_THREADS + threadIdx.x) * W; s < S; s += (i64)gridDim.x * CONF_THREADS * W) {
    float t[W], best[W];
    int idx[W] = {};
    compound_load<W>(t, tg + s);
    compound_load<W>(best, pb + s);
#pragma unroll
    for (int c = 1; c < CT; ++c)
      if (CT <= 5 || c < C) {
        float p[W];
        compound_load<W>(p, pb + (i64)c * S + s);
#pragma unroll
        for (int j = 0; j < W; ++j)
          if (p[j] > best[j]) { best[j] = p[j]; idx[j] = c; }
      }
    conf_voxel<CT>(a, t[0], idx[0], C, ignore);
    if constexpr (W == 4) {   // written out: as a loop over j, CT = 16 keeps 32 more registers live
      conf_voxel<CT>(a, t[1], idx[1], C, ignore);
      conf_voxel<CT>(a, t[2], idx[2], C, ignore);
      conf_voxel<CT>(a, t[3], idx[3], C, ignore);
    }
  }
  conf_commit<CT>(a, C, counts);
}

// two workgroups of 16 waves per compute unit over the whole batch; the grid-stride loop takes the rest
static inline dim3 conf_grid(long long S, int N, bool vec) {
  const i64 items = vec ? S / 4 : S;
  i64 gx = (items + CONF_THREADS - 1) / CONF_THREADS;
  i64 cap = (2 * (i64)seg3d_device_cus() + N - 1) / N;
  if (cap < 1) cap = 1;
  if (gx > cap) gx = cap;
  return dim3((unsigned)gx, (unsigned)N);
}

#define CONF_LAUNCH(CT, VEC) \
  confusion_counts_kernel<CT, VEC><<<grid, dim3(CONF_THREADS), 0, s>>>(probs, target, out, C, (i64)S, ignore_label)

// counts[3c..3c+2] += (tp, fp, fn) of class c over probs [N][C][S] / target [N][S]; `counts` (3 * C int64, device) is owned
// and zeroed by the caller, so that a whole validation pass accumulates on the device.  No allocation, no synchronisation.
extern "C" int seg3d_confusion_counts(const float* probs, const float* target, long long* counts, int N, int C, long long S,
                                      float ignore_label, void* stream) {
  SEG3D_REQUIRE(probs && target && counts, "seg3d_confusion_counts: null pointer");
  SEG3D_REQUIRE(N > 0 && N <= 65535 && S > 0 && S < (1ll << 33), "seg3d_confusion_counts: bad sizes (N = %d, S = %lld)", N, S);
  SEG3D_REQUIRE(C >= 1 && C <= SEG3D_MAXC, "seg3d_confusion_counts: num_class %d not in [1, %d]", C, SEG3D_MAXC);
  const bool vec = compound_vec_ok(S, probs, target, probs);
  const dim3 grid = conf_grid(S, N, vec);
  unsigned long long* out = reinterpret_cast<unsigned long long*>(counts);
  hipStream_t s = (hipStream_t)stream;
  switch (C) {
    case 1: if (vec) CONF_LAUNCH(1, true); else CONF_LAUNCH(1, false); break;
    case 2: if (vec) CONF_LAUNCH(2, true); else CONF_LAUNCH(2, false); break;
    case 3: if (vec) CONF_LAUNCH(3, true); else CONF_LAUNCH(3, false); break;
    case 4: if (vec) CONF_LAUNCH(4, true); else CONF_LAUNCH(4, false); break;
    case 5: if (vec) CONF_LAUNCH(5, true); else CONF_LAUNCH(5, false); break;
    default: if (vec) CONF_LAUNCH(SEG3D_MAXC, true); else CONF_LAUNCH(SEG3D_MAXC, false); break;
  }
  SEG3D_LAUNCH_CHECK("seg3d_confusion_counts");
  return SEG3D_OK;
}

// ---- region-based models: per-region confusion counts of sigmoid probabilities -------------
// The same pass with a threshold in place of the arg-max and set membership in place of class equality: the prediction of
// region r is p_r > 0.5 STRICTLY (inference's rule, seg3d_finalize_regions), its target bit r of the voxel's table word, and a
// voxel counts by the region loss's rule (region_device.h).  A voxel that does not count has no prediction and no target.
template <int CT, bool VEC>
__global__ __launch_bounds__(CONF_THREADS) void region_confusion_counts_kernel(const float* __restrict__ probs,
                                                                                const float* __restrict__ target,
                                                                                RegionLut table,
                                                                                unsigned long long* __restrict__ counts, int R,
                                                                                i64 S, float ignore) {
  const unsigned* lut = table.stage();
  const int n = blockIdx.y;
  const float* tg = target + (i64)n * S;
  const float* pb = probs + (i64)n * R * S;
  ConfAcc<CT> a;
#pragma unroll
  for (int r = 0; r < CT; ++r) a.tp[r] = a.fp[r] = a.fn[r] = 0u;
  constexpr int W = VEC ? 4 : 1;
  for (i64 s = ((i64)blockIdx.x * CONF_THREADS + threadIdx.x) * W; s < S; s += (i64)gridDim.x * CONF_THREADS * W) {
    float t[W];
    int bits[W];
    compound_load<W>(t, tg + s);
#pragma unroll
    for (int j = 0; j < W; ++j) bits[j] = region_bits(lut, t[j], ignore);
#pragma unroll
    for (int r = 0; r < CT; ++r)
      if (CT <= 5 || r < R) {
        float p[W];
        compound_load<W>(p, pb + (i64)r * S + s);
#pragma unroll
        for (int j = 0; j < W; ++j) {
          const bool ok = bits[j] >= 0, pred = ok && p[j] > 0.5f, g = ok && ((bits[j] >> r) & 1);
          a.tp[r] += (pred && g) ? 1u : 0u;
          a.fp[r] += (pred && !g) ? 1u : 0u;
          a.fn[r] += (!pred && g) ? 1u : 0u;
        }
      }
  }
  conf_commit<CT>(a, R, counts);
}

// counts[3r..3r+2] += (tp, fp, fn) of region r over probs [N][R][S] / target [N][S]; `counts` (3 * R int64, device) is owned
// and zeroed by the caller.  lut_host: 256 host words, bit r of lut_host[l] set iff label l is in region r.  No allocation, no
// synchronisation.
extern "C" int seg3d_region_confusion_counts(const float* probs, const float* target, const unsigned* lut_host,
                                             long long* counts, int N, int R, long long S, float ignore_label, void* stream) {
  SEG3D_REQUIRE(probs && target && lut_host && counts, "seg3d_region_confusion_counts: null pointer");
  SEG3D_REQUIRE(N > 0 && N <= 65535 && S > 0 && S < (1ll << 33), "seg3d_region_confusion_counts: bad sizes (N = %d, S = %lld)",
                N, S);
  SEG3D_REQUIRE(R >= 1 && R <= SEG3D_MAXC, "seg3d_region_confusion_counts: %d regions not in [1, %d]", R, SEG3D_MAXC);
  const bool vec = compound_vec_ok(S, probs, target, probs);
  const RegionLut table = region_table(lut_host);
  COMPOUND_DISPATCH(region_confusion_counts_kernel, R, vec,
                    <<<conf_grid(S, N, vec), dim3(CONF_THREADS), 0, (hipStream_t)stream>>>(
                        probs, target, table, reinterpret_cast<unsigned long long*>(counts), R, (i64)S, ignore_label));
  SEG3D_LAUNCH_CHECK("seg3d_region_confusion_counts");
  return SEG3D_OK;
}
