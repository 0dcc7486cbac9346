// topk_loss.hip -- soft Dice + top-k cross-entropy on probabilities, forward + backward (no counterpart in the reference;
// nnU-Net's DC_and_topk_loss; definitions in DESIGN.md section 7, row f15, and include/seg3d_hip.h).
//   counted voxel and L_region:  the compound loss family's (compound_device.h)
//   ell_v = a_t (-log max(p_t, 1e-12)) in fp32 on counted voxels, stored as +0.0 when it is not > 0
//   n = #counted,  k = max(1, (long long)((double)n * k_percent / 100.0))  (n = 0: k = 0, L_topk = 0)
//   tau = k-th largest ell,  m = #{ell > tau},  n_eq = #{ell == tau},  r = k - m
//   L_topk = (sum_{ell > tau} ell + r tau) / k,   L = dice_weight L_region + ce_weight L_topk
//   dL_topk/dp_t = w_v / k * (p_t >= 1e-12 ? -a_t / p_t : 0),  w_v = 1 above tau, r / n_eq at tau, 0 below
// The k-th largest value comes from a three-level radix select (11 / 11 / 10 bits, most significant first) on the bit
// pattern of ell: ell >= 0, so the unsigned order of the bits is the order of the values.  Everything the select decides
// -- n, k, the prefix found so far, the places still to fill -- lives in a device control block; the host reads nothing
// back and bakes nothing data-dependent into a launch, so a captured graph replays correctly on other contents.
// Launches of one forward (ordered by the kernel boundaries only: no flags, tickets or spin-waits):
//   zero (control block + histograms) -> pass A (Dice partial sums, ell) -> 3 x (histogram of one digit over the voxels
//   whose higher digits match the prefix; one-workgroup scan that picks the digit) -> sum of ell above tau, one fp64 slot
//   per workgroup -> one-workgroup fp64 finalize in fixed order.
// Level 1 is NOT fused into pass A: pass A keeps the compound loss's one-workgroup-per-4096-voxels layout (the finalize
// rule of the region term is defined on it), and a 2048-bin flush per such small workgroup would cost about one global
// atomic per two voxels.  The histogram passes run ~2 workgroups per CU over the ell buffer instead (4 bytes per voxel),
// which bounds the global atomics by workgroups x bins.  Integer atomics only: every result is bit-reproducible.
// Bin indices are masked key bits and every loop bound is a size, never a value: NaN or p > 1 cannot leave the arrays.
#include "seg3d_common.h"
#include "seg3d_hip.h"
#include "compound_device.h"

#define TOPK_SENTINEL (-1.0f)      // ell of a voxel that does not count: sign bit set, matches no prefix
#define TOPK_BINS 2048             // bins of one histogram level (level 3 uses the first 1024)
#define TOPK_SHIFT1 21             // level 1: bits 31..21 (bit 31 = sign = 0 on counted voxels), level 2: 20..10, level 3: 9..0
#define TOPK_SHIFT2 10
#define TOPK_MAX_GRID (2 * SEG3D_NUM_CUS)   // workgroups of a histogram / sum pass = fp64 sum slots in the workspace
// control block: 8 int64 words
#define TOPK_N 0
#define TOPK_K 1
#define TOPK_M 2        // voxels above the prefix found so far (after level 3: m)
#define TOPK_NEQ 3      // size of the bin last chosen (after level 3: n_eq)
#define TOPK_LEFT 4     // places still to fill inside that bin (after level 3: r)
#define TOPK_PREFIX 5   // key bits found so far (after level 3: the bits of tau)
#define TOPK_CTRL_WORDS 8
#define TOPK_CTRL_BYTES (TOPK_CTRL_WORDS * 8)
#define TOPK_HIST_BYTES (3 * TOPK_BINS * 4)
#define TOPK_SLOT_BYTES (TOPK_MAX_GRID * 8)

// the entry's own counters start from zero at every call, a replay of a captured graph included
__global__ __launch_bounds__(256) void topk_zero_kernel(unsigned* __restrict__ words, int n) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) words[i] = 0u;
}

// ell of one voxel (sentinel if it does not count); the region sums of `a` take the voxel through the compound loss's code
template <int CT>
__device__ __forceinline__ float topk_voxel(CompoundAcc<CT>& a, float t, const float (&p)[CT], const float (&alpha)[CT], int C,
                                            float ignore) {
  float pt, at;
  if (!compound_region_voxel<CT>(a, t, p, alpha, C, ignore, pt, at)) return TOPK_SENTINEL;
  const float l = at * compound_dist(fmaxf(pt, COMPOUND_PMIN), 0.0f);
  return l > 0.0f ? l : 0.0f;   // -0.0 (p_t == 1) -> +0.0; out of contract (p_t > 1, NaN) -> +0.0 as well
}

// pass A: the (I, P, T) triples of part (its two trailing slots are 0) and ell[n][s]
template <int CT, bool VEC>
__global__ __launch_bounds__(256) void topk_partial_kernel(const float* __restrict__ probs, const float* __restrict__ target,
                                                             const float* __restrict__ alpha_g, float* __restrict__ part,
                                                             float* __restrict__ ell, int C, i64 S, int nblk, float ignore) {
  constexpr int W = VEC ? 4 : 1;
  __shared__ float red[4 * 3];
  float* eb = ell + (i64)blockIdx.y * S;
  float alpha[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) alpha[c] = (CT <= 5 || c < C) ? alpha_g[c] : 0.f;
  CompoundAcc<CT> a;
  compound_block_walk<CT, W>(probs, target, C, S, [&](i64 s, const float (&t)[W], const float (&p)[W][CT]) {
    float e[W];
#pragma unroll
    for (int j = 0; j < W; ++j) e[j] = topk_voxel<CT>(a, t[j], p[j], alpha, C, ignore);
    compound_store<W>(eb + s, e);
  });
  float* dst = compound_region_store<CT>(a, part, C, nblk, red);
  if (threadIdx.x == 0) { dst[3 * C + 0] = 0.f; dst[3 * C + 1] = 0.f; }
}

// One digit's histogram over the keys whose higher digits equal the prefix in the control block (level 1: over every key
// with a clear sign bit).  LDS histogram, then one global atomic per non-zero bin.  nvec = total / 4 when the key buffer
// is 16-byte aligned (16-byte loads + a scalar tail), else 0.
template <int LEVEL>
__device__ __forceinline__ void topk_count_key(unsigned* h, unsigned key, unsigned prefix) {
  if (LEVEL == 1) {
    if ((key >> 31) == 0u) atomicAdd(&h[key >> TOPK_SHIFT1], 1u);                       // < 1024
  } else if (LEVEL == 2) {
    if ((key >> TOPK_SHIFT1) == (prefix >> TOPK_SHIFT1)) atomicAdd(&h[(key >> TOPK_SHIFT2) & (TOPK_BINS - 1)], 1u);
  } else {
    if ((key >> TOPK_SHIFT2) == (prefix >> TOPK_SHIFT2)) atomicAdd(&h[key & ((1u << TOPK_SHIFT2) - 1)], 1u);
  }
}

template <int LEVEL>
__global__ __launch_bounds__(256) void topk_hist_kernel(const unsigned* __restrict__ keys, i64 total, i64 nvec,
                                                          const i64* __restrict__ ctrl, unsigned* __restrict__ hist) {
  __shared__ unsigned h[TOPK_BINS];
  for (int b = threadIdx.x; b < TOPK_BINS; b += 256) h[b] = 0u;
  const unsigned prefix = LEVEL == 1 ? 0u : (unsigned)ctrl[TOPK_PREFIX];   // sign bit always clear
  __syncthreads();
  const i64 tid = (i64)blockIdx.x * 256 + threadIdx.x, stride = (i64)gridDim.x * 256;
  for (i64 i = tid; i < nvec; i += stride) {
    const uint4 k4 = reinterpret_cast<const uint4*>(keys)[i];
    topk_count_key<LEVEL>(h, k4.x, prefix);
    topk_count_key<LEVEL>(h, k4.y, prefix);
    topk_count_key<LEVEL>(h, k4.z, prefix);
    topk_count_key<LEVEL>(h, k4.w, prefix);
  }
  for (i64 i = nvec * 4 + tid; i < total; i += stride) topk_count_key<LEVEL>(h, keys[i], prefix);
  __syncthreads();
  for (int b = threadIdx.x; b < TOPK_BINS; b += 256) {
    const unsigned v = h[b];
    if (v != 0u) atomicAdd(&hist[b], v);
  }
}

// One workgroup: walk this level's bins from the top and pick the digit in whose bin the places left run out; update the
// control block.  Level 1 first derives n (all bins) and k.  Thread j owns the PER bins below BINS - j * PER.
template <int LEVEL>
__global__ __launch_bounds__(256) void topk_scan_kernel(const unsigned* __restrict__ hist, i64* __restrict__ ctrl,
                                                          double k_percent) {
  constexpr int BINS = LEVEL == 3 ? (1 << TOPK_SHIFT2) : TOPK_BINS, PER = BINS / 256;
  constexpr int SHIFT = LEVEL == 1 ? TOPK_SHIFT1 : (LEVEL == 2 ? TOPK_SHIFT2 : 0);
  __shared__ unsigned long long tot[256];
  const int j = threadIdx.x;
  unsigned c[PER];
  unsigned long long mine = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    c[i] = hist[BINS - 1 - (j * PER + i)];
    mine += c[i];
  }
  tot[j] = mine;
  i64 places = LEVEL == 1 ? 0 : ctrl[TOPK_LEFT];
  const i64 prefix = LEVEL == 1 ? 0 : ctrl[TOPK_PREFIX], m_above = LEVEL == 1 ? 0 : ctrl[TOPK_M];
  __syncthreads();   // also: every thread has read the control block before the one below writes it
  unsigned long long above = 0, all = 0;
  for (int q = 0; q < 256; ++q) {
    const unsigned long long v = tot[q];
    all += v;
    above += q < j ? v : 0ull;
  }
  if (LEVEL == 1) {
    const i64 n = (i64)all;
    i64 k = 0;
    if (n > 0) {
      k = (i64)((double)n * k_percent / 100.0);
      if (k < 1) k = 1;
    }
    places = k;
    if (j == 0) {
      ctrl[TOPK_N] = n;
      ctrl[TOPK_K] = k;
    }
  }
  if (places >= 1 && (i64)above < places && places <= (i64)(above + mine)) {   // exactly one thread when 1 <= places <= all
    int digit = -1;
    unsigned long long run = above, before = 0;
    unsigned cnt = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      if (digit < 0 && places <= (i64)(run + c[i])) {
        digit = BINS - 1 - (j * PER + i);
        before = run;
        cnt = c[i];
      }
      run += c[i];
    }
    ctrl[TOPK_PREFIX] = prefix | ((i64)digit << SHIFT);
    ctrl[TOPK_M] = m_above + (i64)before;
    ctrl[TOPK_NEQ] = (i64)cnt;
    ctrl[TOPK_LEFT] = places - (i64)before;
  }
}

// slots[workgroup] = sum of ell above tau (fp64: the sum is exact to the last bits of the fp32 values it adds)
__global__ __launch_bounds__(256) void topk_sum_kernel(const unsigned* __restrict__ keys, i64 total, i64 nvec,
                                                         const i64* __restrict__ ctrl, double* __restrict__ slots) {
  __shared__ double red[4];
  const int tau = (int)ctrl[TOPK_PREFIX];   // >= 0; a sentinel's bits are a negative int and never above it
  double acc = 0.0;
  const i64 tid = (i64)blockIdx.x * 256 + threadIdx.x, stride = (i64)gridDim.x * 256;
  for (i64 i = tid; i < nvec; i += stride) {
    const uint4 k4 = reinterpret_cast<const uint4*>(keys)[i];
    acc += (int)k4.x > tau ? (double)__uint_as_float(k4.x) : 0.0;
    acc += (int)k4.y > tau ? (double)__uint_as_float(k4.y) : 0.0;
    acc += (int)k4.z > tau ? (double)__uint_as_float(k4.z) : 0.0;
    acc += (int)k4.w > tau ? (double)__uint_as_float(k4.w) : 0.0;
  }
  for (i64 i = nvec * 4 + tid; i < total; i += stride) {
    const unsigned key = keys[i];
    acc += (int)key > tau ? (double)__uint_as_float(key) : 0.0;
  }
  acc = wave_sum_d(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) slots[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// One workgroup, fp64, fixed order: the sum slots, then the compound loss's region rule.  loss[3] = (L, L_region, L_topk);
// coef: [R][C][2] = (A, B) of the region term, then tau, ce_weight / k and ce_weight (r / n_eq) / k (0 when the term is off
// or empty); selection[5] = (n, k, m, n_eq, r); threshold[0] = tau.
__global__ __launch_bounds__(256) void topk_finalize_kernel(const float* __restrict__ part, const float* __restrict__ wdice,
                                                              const double* __restrict__ slots, int nslots,
                                                              const i64* __restrict__ ctrl, float* __restrict__ coef,
                                                              float* __restrict__ loss, i64* __restrict__ selection,
                                                              float* __restrict__ threshold, int N, int C, int nblk,
                                                              int batch_dice, float dice_weight, float ce_weight) {
  __shared__ double red[8];
  double above[1];
  compound_column_sum(above, slots, nslots, 1, red);
  const double lr = compound_region_finalize(part, wdice, coef, N, C, nblk, batch_dice, dice_weight, red);
  if (threadIdx.x == 0) {
    const i64 n = ctrl[TOPK_N], k = ctrl[TOPK_K], m = ctrl[TOPK_M], neq = ctrl[TOPK_NEQ], r = ctrl[TOPK_LEFT];
    const float tau = __uint_as_float((unsigned)ctrl[TOPK_PREFIX]);
    const double lt = k > 0 ? (above[0] + (double)r * (double)tau) / (double)k : 0.0;
    double l = 0.0;
    if (dice_weight > 0.f) l += (double)dice_weight * lr;
    if (ce_weight > 0.f) l += (double)ce_weight * lt;
    loss[0] = (float)l;
    loss[1] = (float)lr;
    loss[2] = (float)lt;
    const int R = batch_dice ? 1 : N;
    const bool on = ce_weight > 0.f && k > 0 && neq > 0;
    coef[2 * R * C + 0] = tau;
    coef[2 * R * C + 1] = on ? (float)((double)ce_weight / (double)k) : 0.f;
    coef[2 * R * C + 2] = on ? (float)((double)ce_weight * ((double)r / (double)neq) / (double)k) : 0.f;
    selection[0] = n; selection[1] = k; selection[2] = m; selection[3] = neq; selection[4] = r;
    threshold[0] = tau;
  }
}

// the top-k coefficient of one voxel from its ell bits: a sentinel is below every tau
__device__ __forceinline__ float topk_coef(float e, int tau, float c_above, float c_at) {
  const int key = (int)__float_as_uint(e);
  return key > tau ? c_above : (key == tau ? c_at : 0.f);
}

// the distribution part of compound_voxel_grad (gamma = 0: -1 / p_t) takes each voxel's own coefficient
template <int CT, bool VEC>
__global__ __launch_bounds__(256) void topk_bwd_kernel(const float* __restrict__ probs, const float* __restrict__ target,
                                                         const float* __restrict__ ell, const float* __restrict__ coef,
                                                         const float* __restrict__ alpha_g, const float* __restrict__ gout,
                                                         float* __restrict__ dprobs, int C, i64 S, int R, float ignore) {
  constexpr int W = VEC ? 4 : 1;
  const int tau = (int)__float_as_uint(coef[2 * R * C + 0]);
  const float c_above = coef[2 * R * C + 1], c_at = coef[2 * R * C + 2];
  const float* eb = ell + (i64)blockIdx.y * S;
  compound_bwd_body<CT, W>(probs, target, coef, alpha_g, gout, dprobs, C, S, R, ignore, 0.0f, [&](i64 s, float (&cd)[W]) {
    float e[W];
    compound_load<W>(e, eb + s);
#pragma unroll
    for (int j = 0; j < W; ++j) cd[j] = topk_coef(e[j], tau, c_above, c_at);
  });
}

// control block | three histograms | fp64 sum slots | Dice partial sums
extern "C" long long seg3d_topk_loss_workspace_bytes(int N, int C, long long S) {
  if (N <= 0 || C <= 0 || S <= 0) return 0;
  return (long long)TOPK_CTRL_BYTES + TOPK_HIST_BYTES + TOPK_SLOT_BYTES + seg3d_compound_loss_part_floats(N, C, S) * 4;
}

extern "C" int seg3d_topk_loss_fwd(const float* probs, const float* target, const float* wdice, const float* alpha,
                                   void* workspace, float* ell, float* coef, float* loss, long long* selection,
                                   float* threshold, int N, int C, long long S, double k_percent, float dice_weight,
                                   float ce_weight, int batch_dice, float ignore_label, void* stream) {
  SEG3D_REQUIRE(probs && target && wdice && alpha && workspace && ell && coef && loss && selection && threshold && N > 0 &&
                    N <= 65535 && S > 0,
                "seg3d_topk_loss_fwd: bad arguments");
  SEG3D_REQUIRE(C >= 1 && C <= SEG3D_MAXC, "seg3d_topk_loss_fwd: num_class %d not in [1, %d]", C, SEG3D_MAXC);
  SEG3D_REQUIRE(k_percent > 0.0 && k_percent <= 100.0, "seg3d_topk_loss_fwd: k_percent %g not in (0, 100]", k_percent);
  SEG3D_REQUIRE(dice_weight >= 0.f && ce_weight >= 0.f && (dice_weight > 0.f || ce_weight > 0.f),
                "seg3d_topk_loss_fwd: the term weights must be >= 0 and not both 0");
  const i64 total = (i64)N * S;
  SEG3D_REQUIRE(total < (1ll << 32), "seg3d_topk_loss_fwd: %lld voxels do not fit the 32-bit histogram counters", total);
  SEG3D_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)selection & 7) == 0,
                "seg3d_topk_loss_fwd: workspace and selection must be 8-byte aligned");
  char* ws = reinterpret_cast<char*>(workspace);
  i64* ctrl = reinterpret_cast<i64*>(ws);
  unsigned* hist = reinterpret_cast<unsigned*>(ws + TOPK_CTRL_BYTES);
  double* slots = reinterpret_cast<double*>(ws + TOPK_CTRL_BYTES + TOPK_HIST_BYTES);
  float* part = reinterpret_cast<float*>(ws + TOPK_CTRL_BYTES + TOPK_HIST_BYTES + TOPK_SLOT_BYTES);
  const unsigned* keys = reinterpret_cast<const unsigned*>(ell);
  hipStream_t s = (hipStream_t)stream;
  const int nzero = (TOPK_CTRL_BYTES + TOPK_HIST_BYTES) / 4;
  topk_zero_kernel<<<dim3((nzero + 255) / 256), dim3(256), 0, s>>>(reinterpret_cast<unsigned*>(ws), nzero);
  SEG3D_LAUNCH_CHECK("seg3d_topk_loss_fwd(zero)");
  const int nblk = (int)seg3d_dice_blocks(S);
  const bool vec = compound_vec_ok(S, probs, target, ell);
  COMPOUND_DISPATCH(topk_partial_kernel, C, vec,
                    <<<dim3(nblk, N), dim3(256), 0, s>>>(probs, target, alpha, part, ell, C, (i64)S, nblk, ignore_label));
  SEG3D_LAUNCH_CHECK("seg3d_topk_loss_fwd(partial)");
  // two workgroups per compute unit over the whole ell buffer; the grid-stride loop takes the rest
  const i64 nvec = ((uintptr_t)ell & 15) == 0 ? total / 4 : 0;
  i64 g = ((nvec ? nvec : total) + 255) / 256, cap = 2 * (i64)seg3d_device_cus();
  if (cap > TOPK_MAX_GRID) cap = TOPK_MAX_GRID;
  if (g > cap) g = cap;
  const dim3 grid((unsigned)g);
  topk_hist_kernel<1><<<grid, dim3(256), 0, s>>>(keys, total, nvec, ctrl, hist);
  topk_scan_kernel<1><<<dim3(1), dim3(256), 0, s>>>(hist, ctrl, k_percent);
  topk_hist_kernel<2><<<grid, dim3(256), 0, s>>>(keys, total, nvec, ctrl, hist + TOPK_BINS);
  topk_scan_kernel<2><<<dim3(1), dim3(256), 0, s>>>(hist + TOPK_BINS, ctrl, k_percent);
  topk_hist_kernel<3><<<grid, dim3(256), 0, s>>>(keys, total, nvec, ctrl, hist + 2 * TOPK_BINS);
  topk_scan_kernel<3><<<dim3(1), dim3(256), 0, s>>>(hist + 2 * TOPK_BINS, ctrl, k_percent);
  SEG3D_LAUNCH_CHECK("seg3d_topk_loss_fwd(select)");
  topk_sum_kernel<<<grid, dim3(256), 0, s>>>(keys, total, nvec, ctrl, slots);
  SEG3D_LAUNCH_CHECK("seg3d_topk_loss_fwd(sum)");
  topk_finalize_kernel<<<dim3(1), dim3(256), 0, s>>>(part, wdice, slots, (int)g, ctrl, coef, loss, selection, threshold, N, C,
                                                     nblk, batch_dice ? 1 : 0, dice_weight, ce_weight);
  SEG3D_LAUNCH_CHECK("seg3d_topk_loss_fwd(finalize)");
  return SEG3D_OK;
}

extern "C" int seg3d_topk_loss_bwd(const float* probs, const float* target, const float* ell, const float* coef,
                                   const float* alpha, const float* gout, float* dprobs, int N, int C, long long S,
                                   int batch_dice, float ignore_label, void* stream) {
  SEG3D_REQUIRE(probs && target && ell && coef && alpha && gout && dprobs && N > 0 && N <= 65535 && S > 0,
                "seg3d_topk_loss_bwd: bad arguments");
  SEG3D_REQUIRE(C >= 1 && C <= SEG3D_MAXC, "seg3d_topk_loss_bwd: num_class %d not in [1, %d]", C, SEG3D_MAXC);
  const bool vec = compound_vec_ok(S, probs, target, dprobs) && ((uintptr_t)ell & 15) == 0;
  const int R = batch_dice ? 1 : N;
  COMPOUND_DISPATCH(topk_bwd_kernel, C, vec,
                    <<<compound_bwd_grid(S, N, vec), dim3(256), 0, (hipStream_t)stream>>>(probs, target, ell, coef, alpha, gout,
                                                                                         dprobs, C, (i64)S, R, ignore_label));
  SEG3D_LAUNCH_CHECK("seg3d_topk_loss_bwd");
  return SEG3D_OK;
}
