// volume_stats.hip -- exact statistics of whole volumes for case-level intensity normalisation (no counterpart in the
// reference; nnU-Net's ZScoreNormalization / CTNormalization need them; definitions in DESIGN.md section 7 row f20 and
// include/seg3d_hip.h).
//   volume [Z][Y][X][M] fp32 channels-last, M <= 8; optional selection plane sel [Z][Y][X] uint8
//   S_m = all voxels (mode 0) | x != 0 by its bits, so -0.0 is out and a denormal is in (mode 1) | sel[v] != 0 (mode 2)
//   per modality: n = |S_m|, min, max, up to 4 order statistics sorted(S_m)[floor(q (n - 1) + 0.5)], mean and population
//   std in fp64 (std floored at 1e-6), optionally of the values clamped to [value(q_0), value(q_1)]
// Order statistics: three-level radix select (11 / 11 / 10 bits, most significant first, as topk_loss.hip) over the
// order-preserving key of the float: negatives have all bits flipped, the others get the sign bit set, -0.0 is keyed (and
// reported) as +0.0.  Level 0 keeps one histogram per modality, shared by its ranks; levels 1 and 2 one per (modality,
// rank) over the keys whose higher digits match that rank's prefix.  Equal ranks are resolved once (the later one is an
// alias).  Everything the select decides lives in the state's control block: the host reads nothing back between the
// passes and bakes nothing data-dependent into a launch.
// Histogram pass: LDS-private histograms per workgroup, non-zero bins flushed with one 64-bit global atomic each (the
// global bins are 64-bit so that a data set may be accumulated; the LDS bins hold one call's < 2^31 voxels).  Lanes of a
// wave that hit the same bin are collapsed before the LDS atomic as in lesion.hip's pair pass, but for at most
// VS_ROUNDS leaders: a CT background (one value in most lanes) costs one atomic per wave, while uniform data -- 64
// distinct bins per wave, where a full collapse would take 64 rounds -- pays two ballots and falls through to one atomic
// per lane.
// Moments: d = x - pivot in fp64 (pivot = midpoint of the value range in use, so an all-equal volume gives exactly 0),
// sum d and sum d^2, one slot pair per (workgroup, modality); a further volume adds to the same slots (only workgroup b
// touches slot b, launches are stream-ordered).  The finish kernel adds the slots in a fixed order.  Integer atomics only:
// two runs are bit-equal.
// Every bin index is masked key bits and every loop bound is a size: NaN / Inf cannot leave the arrays.
#include "mc_device.h"
#include "seg3d_hip.h"

#define VS_MAXM 8
#define VS_MAXQ 4
#define VS_BINS 2048             // bins of levels 0 and 1 (level 2 uses the first 1024)
#define VS_SHIFT0 21             // level 0: bits 31..21, level 1: 20..10, level 2: 9..0
#define VS_SHIFT1 10
// Histogram passes: at most two workgroups of 1024 threads per CU (32 waves; 32 KB of LDS each).  Wide workgroups, not more
// of them: the flush costs workgroups x non-zero bins 64-bit global atomics, the loads want many waves in flight.
#define VS_HIST_THREADS 1024
#define VS_HIST_GRID (2 * SEG3D_NUM_CUS)
#define VS_MAX_GRID (8 * SEG3D_NUM_CUS)   // workgroups of a moments pass (256 threads) = moment slots in the state
#define VS_UNROLL 4              // rows a thread has in flight per step
#define VS_ROUNDS 2              // leaders collapsed per wave before the per-lane atomics
// control block: VS_CW int64 words per modality
#define VS_N 0
#define VS_MINKEY 1
#define VS_MAXKEY 2
#define VS_RANK 4                // + q: the rank k_q
#define VS_PREFIX 8              // + q: key bits found so far (after level 2: the key of the order statistic)
#define VS_LEFT 12               // + q: rank inside the bin last chosen
#define VS_ALIAS 16              // + q: -1 = resolved on its own, q' < q = same rank as q', -2 = off (q >= Q or n == 0)
#define VS_CW 32
#define VS_CTRL_BYTES (VS_MAXM * VS_CW * 8)
#define VS_OUT 9                 // doubles per modality: n, min, max, mean, std, q_0..q_3

typedef unsigned long long u64;

static inline i64 vs_hist0_words(int M) { return (i64)M * VS_BINS; }
static inline i64 vs_hist1_words(int M) { return (i64)M * VS_MAXQ * VS_BINS; }
static inline i64 vs_hist2_words(int M) { return (i64)M * VS_MAXQ * (VS_BINS / 2); }
static inline i64 vs_slot_words(int M) { return (i64)VS_MAX_GRID * M * 2; }

__device__ __forceinline__ unsigned vs_key(unsigned bits) {
  if (bits == 0x80000000u) bits = 0u;
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
__device__ __forceinline__ unsigned vs_unkey(unsigned key) { return (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key; }
// exact whatever the fp32 denormal mode of the conversion instruction
__device__ __forceinline__ double vs_double(unsigned bits) {
  if (((bits >> 23) & 0xffu) == 0u) {
    const double d = (double)(int)(bits & 0x7fffffu) * 0x1p-149;
    return (bits >> 31) ? -d : d;
  }
  return (double)__uint_as_float(bits);
}
__device__ __forceinline__ bool vs_selected(int mode, unsigned bits, unsigned char s) {
  return mode == 0 ? true : (mode == 1 ? (bits & 0x7fffffffu) != 0u : s != 0);
}

// h[bin] += 1 for the lanes that are `on`; called by whole waves (uniform control flow)
__device__ __forceinline__ void vs_count(unsigned* h, bool on, unsigned bin) {
  const int lane = threadIdx.x & 63;
  u64 todo = __ballot(on);
#pragma unroll
  for (int r = 0; r < VS_ROUNDS; ++r) {
    if (!todo) break;   // uniform over the wave
    const int leader = __ffsll(todo) - 1;   // uniform: the leader's bin comes through a scalar register, not through LDS
    const unsigned b = (unsigned)__builtin_amdgcn_readlane((int)bin, leader);
    const u64 same = __ballot(on && bin == b) & todo;
    if (lane == leader) atomicAdd(&h[b], (unsigned)__popcll(same));
    todo &= ~same;
  }
  if ((todo >> lane) & 1ull) atomicAdd(&h[bin], 1u);
}

// the value range the moments are taken over (keys) and the pivot; clip: [value(q_0), value(q_1)], else [min, max]
__device__ __forceinline__ void vs_bounds(const i64* __restrict__ c, int clip, unsigned& klo, unsigned& khi, double& pivot) {
  if (c[VS_N] <= 0) {
    klo = 0u; khi = 0xffffffffu; pivot = 0.0;
    return;
  }
  if (clip) {
    const i64 a0 = c[VS_ALIAS + 0], a1 = c[VS_ALIAS + 1];
    klo = (unsigned)c[VS_PREFIX + (a0 >= 0 && a0 < VS_MAXQ ? (int)a0 : 0)];
    khi = (unsigned)c[VS_PREFIX + (a1 >= 0 && a1 < VS_MAXQ ? (int)a1 : 1)];
  } else {
    klo = (unsigned)c[VS_MINKEY];
    khi = (unsigned)c[VS_MAXKEY];
  }
  pivot = 0.5 * (vs_double(vs_unkey(klo)) + vs_double(vs_unkey(khi)));
}

__global__ __launch_bounds__(256) void vs_begin_kernel(u64* __restrict__ words, i64 n) {
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256)
    words[i] = (i < VS_MAXM * VS_CW && (i % VS_CW) == VS_MINKEY) ? 0xffffffffull : 0ull;
}

// LEVEL 0: blockIdx.y = group of four modalities, h[j] = histogram of the top digit of modality 4 y + j, and min / max.
// LEVEL 1, 2: blockIdx.y = modality, h[q] = histogram of this level's digit over the keys that match rank q's prefix.
template <int MC, bool VEC, int LEVEL>
__global__ __launch_bounds__(VS_HIST_THREADS) void vs_hist_kernel(const float* __restrict__ vol,
                                                                    const unsigned char* __restrict__ sel, i64 nv, int Mrt,
                                                                    int mode, i64* __restrict__ ctrl, u64* __restrict__ hist) {
  constexpr int MR = mc_regs<MC>;
  constexpr int BINS = LEVEL == 2 ? VS_BINS / 2 : VS_BINS;
  constexpr int T = VS_HIST_THREADS;
  const int M = mc_width<MC>(Mrt);
  __shared__ unsigned h[4 * VS_BINS];
  __shared__ unsigned smin[4], smax[4];
  for (int b = threadIdx.x; b < 4 * VS_BINS; b += T) h[b] = 0u;
  if (threadIdx.x < 4) {
    smin[threadIdx.x] = 0xffffffffu;
    smax[threadIdx.x] = 0u;
  }
  const int g = blockIdx.y;
  bool act[VS_MAXQ] = {false, false, false, false};
  unsigned prefix[VS_MAXQ] = {0u, 0u, 0u, 0u};
  bool any = LEVEL == 0;
  if (LEVEL > 0) {
#pragma unroll
    for (int q = 0; q < VS_MAXQ; ++q) {
      act[q] = ctrl[g * VS_CW + VS_ALIAS + q] == -1;
      prefix[q] = (unsigned)ctrl[g * VS_CW + VS_PREFIX + q];
      any = any || act[q];
    }
  }
  unsigned kmn[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, kmx[4] = {0u, 0u, 0u, 0u};
  __syncthreads();
  if (any) {   // uniform over the workgroup
    for (i64 base = (i64)blockIdx.x * (T * VS_UNROLL); base < nv; base += (i64)gridDim.x * (T * VS_UNROLL)) {
      float r[VS_UNROLL][MR];
      unsigned char s[VS_UNROLL];
      bool in[VS_UNROLL];
#pragma unroll
      for (int u = 0; u < VS_UNROLL; ++u) {
        const i64 v = base + u * T + threadIdx.x;
        in[u] = v < nv;
        s[u] = 1;
        if (in[u]) {
          mc_load_row<MC, VEC>(vol + v * M, r[u], M, 0.f);
          if (mode == 2) s[u] = sel[v];
        } else {
#pragma unroll
          for (int m = 0; m < MR; ++m) r[u][m] = 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < VS_UNROLL; ++u) {
        if (LEVEL == 0) {
#pragma unroll
          for (int m = 0; m < MR; ++m) {
            if (MC == 0 && ((m >> 2) != g || m >= M)) continue;   // uniform
            const unsigned bits = __float_as_uint(r[u][m]);
            const bool on = in[u] && vs_selected(mode, bits, s[u]);
            const unsigned key = vs_key(bits);
            if (on) {
              kmn[m & 3] = key < kmn[m & 3] ? key : kmn[m & 3];
              kmx[m & 3] = key > kmx[m & 3] ? key : kmx[m & 3];
            }
            vs_count(h + (m & 3) * VS_BINS, on, key >> VS_SHIFT0);
          }
        } else {
          float x = r[u][0];
#pragma unroll
          for (int m = 1; m < MR; ++m) x = m == g ? r[u][m] : x;
          const unsigned bits = __float_as_uint(x);
          const bool on = in[u] && vs_selected(mode, bits, s[u]);
          const unsigned key = vs_key(bits);
#pragma unroll
          for (int q = 0; q < VS_MAXQ; ++q) {
            if (!act[q]) continue;   // uniform
            if (LEVEL == 1)
              vs_count(h + q * VS_BINS, on && (key >> VS_SHIFT0) == (prefix[q] >> VS_SHIFT0),
                       (key >> VS_SHIFT1) & (VS_BINS - 1));
            else
              vs_count(h + q * VS_BINS, on && (key >> VS_SHIFT1) == (prefix[q] >> VS_SHIFT1),
                       key & ((1u << VS_SHIFT1) - 1));
          }
        }
      }
    }
  }
  if (LEVEL == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      atomicMin(&smin[j], kmn[j]);
      atomicMax(&smax[j], kmx[j]);
    }
  }
  __syncthreads();
  // level 0: row j of h belongs to modality 4 g + j; levels 1, 2: row q to (modality g, rank q)
  for (int i = threadIdx.x; i < 4 * BINS; i += T) {
    const int row = i / BINS, b = i - row * BINS;
    const unsigned v = h[row * VS_BINS + b];
    if (v == 0u) continue;
    if (LEVEL == 0) {
      const int m = 4 * g + row;
      if (m < M) atomicAdd(&hist[(i64)m * VS_BINS + b], (u64)v);
    } else {
      atomicAdd(&hist[((i64)g * VS_MAXQ + row) * BINS + b], (u64)v);
    }
  }
  if (LEVEL == 0 && threadIdx.x < 4) {
    const int m = 4 * g + threadIdx.x;
    if (m < M && smin[threadIdx.x] <= smax[threadIdx.x]) {   // this workgroup saw a selected voxel of m
      atomicMin(reinterpret_cast<u64*>(ctrl + m * VS_CW + VS_MINKEY), (u64)smin[threadIdx.x]);
      atomicMax(reinterpret_cast<u64*>(ctrl + m * VS_CW + VS_MAXKEY), (u64)smax[threadIdx.x]);
    }
  }
}

struct VsQuantiles {
  double q[VS_MAXQ];
};

// One workgroup per (modality blockIdx.x, rank blockIdx.y): walk this level's bins from the bottom and pick the digit in
// whose bin the rank falls.  Level 0 first derives n and every rank k_q = floor(q (n - 1) + 0.5) in double (each rank's
// workgroup does so for itself: no workgroup reads what another one writes).  Thread j owns the PER bins from j * PER.
template <int LEVEL>
__global__ __launch_bounds__(256) void vs_resolve_kernel(const u64* __restrict__ hist, i64* __restrict__ ctrl, int Q,
                                                           VsQuantiles qs) {
  constexpr int BINS = LEVEL == 2 ? VS_BINS / 2 : VS_BINS, PER = BINS / 256;
  constexpr int SHIFT = LEVEL == 0 ? VS_SHIFT0 : (LEVEL == 1 ? VS_SHIFT1 : 0);
  __shared__ u64 tot[256];
  const int m = blockIdx.x, q = blockIdx.y, j = threadIdx.x;
  i64* c = ctrl + m * VS_CW;
  if (LEVEL > 0 && c[VS_ALIAS + q] != -1) return;   // uniform, before any barrier; nobody writes this word at this level
  const u64* hb = LEVEL == 0 ? hist + (i64)m * BINS : hist + ((i64)m * VS_MAXQ + q) * BINS;
  u64 cnt[PER], mine = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    cnt[i] = hb[j * PER + i];
    mine += cnt[i];
  }
  tot[j] = mine;
  i64 rank = LEVEL == 0 ? 0 : c[VS_LEFT + q];
  const i64 prefix = LEVEL == 0 ? 0 : c[VS_PREFIX + q];
  __syncthreads();   // also: every thread has read the control block before the one below writes it
  u64 below = 0, all = 0;
  for (int t = 0; t < 256; ++t) {
    const u64 v = tot[t];
    all += v;
    below += t < j ? v : 0ull;
  }
  if (LEVEL == 0) {
    const i64 n = (i64)all;
    i64 alias = -2;
    if (q < Q && n > 0) {
      i64 k[VS_MAXQ];
#pragma unroll
      for (int t = 0; t < VS_MAXQ; ++t) {
        i64 kt = (i64)floor(qs.q[t] * (double)(n - 1) + 0.5);
        k[t] = kt < 0 ? 0 : (kt > n - 1 ? n - 1 : kt);
      }
      alias = -1;
#pragma unroll
      for (int t = VS_MAXQ - 1; t >= 0; --t)
        if (t < q && k[t] == k[q]) alias = t;   // the first rank with the same k
      rank = k[q];
    }
    if (j == 0) {
      if (q == 0) c[VS_N] = n;
      c[VS_ALIAS + q] = alias;
      c[VS_RANK + q] = alias == -2 ? -1 : rank;
    }
    if (alias != -1) return;   // uniform; after the only barrier
  }
  if (rank >= (i64)below && rank < (i64)(below + mine)) {   // exactly one thread when 0 <= rank < all
    int digit = -1;
    u64 run = below, before = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      if (digit < 0 && rank < (i64)(run + cnt[i])) {
        digit = j * PER + i;
        before = run;
      }
      run += cnt[i];
    }
    c[VS_PREFIX + q] = prefix | ((i64)digit << SHIFT);
    c[VS_LEFT + q] = rank - (i64)before;
  }
}

// slots[(workgroup * M + m) * 2] += (sum d, sum d^2) over this volume's selected voxels, d = clamp(x) - pivot in fp64
template <int MC, bool VEC>
__global__ __launch_bounds__(256) void vs_moments_kernel(const float* __restrict__ vol, const unsigned char* __restrict__ sel,
                                                           i64 nv, int Mrt, int mode, int clip,
                                                           const i64* __restrict__ ctrl, double* __restrict__ slots) {
  constexpr int MR = mc_regs<MC>;
  const int M = mc_width<MC>(Mrt);
  __shared__ double red[MR][8];
  unsigned klo[MR], khi[MR];
  double pivot[MR], sum[MR], sq[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) {
    sum[m] = sq[m] = 0.0;
    klo[m] = 0u; khi[m] = 0xffffffffu; pivot[m] = 0.0;
    if (m < M) vs_bounds(ctrl + m * VS_CW, clip, klo[m], khi[m], pivot[m]);
  }
  for (i64 base = (i64)blockIdx.x * (256 * VS_UNROLL); base < nv; base += (i64)gridDim.x * (256 * VS_UNROLL)) {
    float r[VS_UNROLL][MR];
    unsigned char s[VS_UNROLL];
    bool in[VS_UNROLL];
#pragma unroll
    for (int u = 0; u < VS_UNROLL; ++u) {
      const i64 v = base + u * 256 + threadIdx.x;
      in[u] = v < nv;
      s[u] = 1;
      if (in[u]) {
        mc_load_row<MC, VEC>(vol + v * M, r[u], M, 0.f);
        if (mode == 2) s[u] = sel[v];
      } else {
#pragma unroll
        for (int m = 0; m < MR; ++m) r[u][m] = 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < VS_UNROLL; ++u) {
#pragma unroll
      for (int m = 0; m < MR; ++m) {
        const unsigned bits = __float_as_uint(r[u][m]);
        const bool on = in[u] && (MC > 0 || m < M) && vs_selected(mode, bits, s[u]);
        unsigned key = vs_key(bits);
        key = key < klo[m] ? klo[m] : (key > khi[m] ? khi[m] : key);
        const double d = on ? vs_double(vs_unkey(key)) - pivot[m] : 0.0;
        sum[m] += d;
        sq[m] += d * d;
      }
    }
  }
  mc_stat_park(sum, red, 0);
  mc_stat_park(sq, red, 4);
  __syncthreads();
  if (threadIdx.x < M) {
    const int m = threadIdx.x;
    double* slot = slots + ((i64)blockIdx.x * M + m) * 2;
    slot[0] += mc_stat_total(red[m]);
    slot[1] += mc_stat_total(red[m] + 4);
  }
}

// One workgroup, fp64, fixed order: thread t adds slots t and t + 256, then a binary tree over the 256 threads.
// out[m][VS_OUT] = n, min, max, mean, std, value(q_0..q_3) (0 past Q); n == 0: all 0 and std = 1e-6.
__global__ __launch_bounds__(256) void vs_finish_kernel(const i64* __restrict__ ctrl, const double* __restrict__ slots,
                                                          int M, int Q, int clip, double* __restrict__ out) {
  __shared__ double red[256];
  for (int m = 0; m < M; ++m) {
    double tot[2];
    for (int k = 0; k < 2; ++k) {
      double a = 0.0;
      for (int b = threadIdx.x; b < VS_MAX_GRID; b += 256) a += slots[((i64)b * M + m) * 2 + k];
      __syncthreads();
      red[threadIdx.x] = a;
      __syncthreads();
      for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
      }
      tot[k] = red[0];
    }
    if (threadIdx.x == 0) {
      const i64* c = ctrl + m * VS_CW;
      double* o = out + m * VS_OUT;
      const i64 n = c[VS_N];
      for (int i = 0; i < VS_OUT; ++i) o[i] = 0.0;
      o[4] = 1e-6;
      if (n > 0) {
        unsigned klo, khi;
        double pivot;
        vs_bounds(c, clip, klo, khi, pivot);
        const double md = tot[0] / (double)n;
        double var = tot[1] / (double)n - md * md;
        if (!(var > 0.0)) var = 0.0;
        double sd = sqrt(var);
        if (!(sd >= 1e-6)) sd = 1e-6;
        o[0] = (double)n;
        o[1] = vs_double(vs_unkey((unsigned)c[VS_MINKEY]));
        o[2] = vs_double(vs_unkey((unsigned)c[VS_MAXKEY]));
        o[3] = pivot + md;
        o[4] = sd;
        for (int q = 0; q < Q && q < VS_MAXQ; ++q) {
          const i64 a = c[VS_ALIAS + q];
          const int src = a >= 0 && a < VS_MAXQ ? (int)a : q;
          o[5 + q] = vs_double(vs_unkey((unsigned)c[VS_PREFIX + src]));
        }
      }
    }
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
// control block | level-0 histograms [M] | level-1 [M][4] | level-2 [M][4] (1024 bins) | moment slots [VS_MAX_GRID][M][2]
extern "C" long long seg3d_volume_stats_state_bytes(int M) {
  if (M < 1 || M > VS_MAXM) return 0;
  return (long long)VS_CTRL_BYTES + 8 * (vs_hist0_words(M) + vs_hist1_words(M) + vs_hist2_words(M) + vs_slot_words(M));
}

struct VsState {
  i64* ctrl;
  u64 *hist0, *hist1, *hist2;
  double* slots;
};
static inline VsState vs_state(void* state, int M) {
  VsState s;
  s.ctrl = reinterpret_cast<i64*>(state);
  s.hist0 = reinterpret_cast<u64*>(state) + VS_MAXM * VS_CW;
  s.hist1 = s.hist0 + vs_hist0_words(M);
  s.hist2 = s.hist1 + vs_hist1_words(M);
  s.slots = reinterpret_cast<double*>(s.hist2 + vs_hist2_words(M));
  return s;
}

#define VS_CHECK_STATE(name)                                                                                        \
  SEG3D_REQUIRE(state && ((uintptr_t)state & 7) == 0, name ": state must be an 8-byte aligned device buffer");      \
  SEG3D_REQUIRE(M >= 1 && M <= VS_MAXM, name ": M = %d modalities, 1..8 are supported", M)
#define VS_CHECK_VOLUME(name)                                                                                       \
  SEG3D_REQUIRE(volume && ((uintptr_t)volume & 3) == 0, name ": volume must be a 4-byte aligned device buffer");    \
  SEG3D_REQUIRE(voxels > 0 && voxels < (1ll << 31), name ": bad voxel count %lld (1 .. 2^31 - 1)", voxels);         \
  SEG3D_REQUIRE(mode >= 0 && mode <= 2, name ": selection mode %d not in 0..2", mode);                              \
  SEG3D_REQUIRE(mode != 2 || sel, name ": mode 2 needs the selection plane")

// workgroups (x) of a pass over nv voxels: `threads` * VS_UNROLL voxels per step, at most per_cu per CU and `most` in all
static inline unsigned vs_grid_x(i64 nv, int threads, int per_cu, i64 most) {
  i64 g = (nv + threads * VS_UNROLL - 1) / (threads * VS_UNROLL), cap = per_cu * (i64)seg3d_device_cus();
  if (cap > most) cap = most;
  if (g > cap) g = cap;
  return (unsigned)(g < 1 ? 1 : g);
}

extern "C" int seg3d_volume_stats_begin(void* state, int M, void* stream) {
  VS_CHECK_STATE("seg3d_volume_stats_begin");
  const i64 words = seg3d_volume_stats_state_bytes(M) / 8;
  vs_begin_kernel<<<dim3(seg3d_ew_grid(words, 256)), dim3(256), 0, (hipStream_t)stream>>>(reinterpret_cast<u64*>(state),
                                                                                          words);
  SEG3D_LAUNCH_CHECK("seg3d_volume_stats_begin");
  return SEG3D_OK;
}

template <int MC, bool VEC>
static void vs_hist_launch(int level, dim3 grid, hipStream_t s, const float* volume, const unsigned char* sel, i64 nv,
                           int M, int mode, const VsState& st) {
  const dim3 block(VS_HIST_THREADS);
  if (level == 0)
    vs_hist_kernel<MC, VEC, 0><<<grid, block, 0, s>>>(volume, sel, nv, M, mode, st.ctrl, st.hist0);
  else if (level == 1)
    vs_hist_kernel<MC, VEC, 1><<<grid, block, 0, s>>>(volume, sel, nv, M, mode, st.ctrl, st.hist1);
  else
    vs_hist_kernel<MC, VEC, 2><<<grid, block, 0, s>>>(volume, sel, nv, M, mode, st.ctrl, st.hist2);
}

extern "C" int seg3d_volume_stats_accumulate_hist(const float* volume, const unsigned char* sel, long long voxels, int M,
                                                  int mode, int level, void* state, void* stream) {
  VS_CHECK_STATE("seg3d_volume_stats_accumulate_hist");
  VS_CHECK_VOLUME("seg3d_volume_stats_accumulate_hist");
  SEG3D_REQUIRE(level >= 0 && level <= 2, "seg3d_volume_stats_accumulate_hist: level %d not in 0..2", level);
  const VsState st = vs_state(state, M);
  const dim3 grid(vs_grid_x(voxels, VS_HIST_THREADS, 2, VS_HIST_GRID), level == 0 ? (unsigned)((M + 3) / 4) : (unsigned)M);
  MC_DISPATCH(vs_hist_launch, M, mc_vec_rows(M, volume),
              (level, grid, (hipStream_t)stream, volume, sel, (i64)voxels, M, mode, st));
  SEG3D_LAUNCH_CHECK("seg3d_volume_stats_accumulate_hist");
  return SEG3D_OK;
}

static int vs_check_quantiles(const char* name, int Q, const double* quantiles, VsQuantiles& qs) {
  SEG3D_REQUIRE(Q >= 0 && Q <= VS_MAXQ, "%s: Q = %d order statistics, 0..4 are supported", name, Q);
  SEG3D_REQUIRE(Q == 0 || quantiles, "%s: Q > 0 needs the quantiles", name);
  for (int q = 0; q < VS_MAXQ; ++q) {
    qs.q[q] = q < Q ? quantiles[q] : 0.0;
    SEG3D_REQUIRE(qs.q[q] >= 0.0 && qs.q[q] <= 1.0, "%s: quantile %g not in [0, 1]", name, qs.q[q]);
  }
  return SEG3D_OK;
}

extern "C" int seg3d_volume_stats_resolve(void* state, int M, int Q, const double* quantiles, int level, void* stream) {
  VS_CHECK_STATE("seg3d_volume_stats_resolve");
  SEG3D_REQUIRE(level >= 0 && level <= 2, "seg3d_volume_stats_resolve: level %d not in 0..2", level);
  VsQuantiles qs;
  const int rc = vs_check_quantiles("seg3d_volume_stats_resolve", Q, quantiles, qs);
  if (rc != SEG3D_OK) return rc;
  const VsState st = vs_state(state, M);
  const dim3 grid(M, VS_MAXQ);
  hipStream_t s = (hipStream_t)stream;
  if (level == 0)
    vs_resolve_kernel<0><<<grid, dim3(256), 0, s>>>(st.hist0, st.ctrl, Q, qs);
  else if (level == 1)
    vs_resolve_kernel<1><<<grid, dim3(256), 0, s>>>(st.hist1, st.ctrl, Q, qs);
  else
    vs_resolve_kernel<2><<<grid, dim3(256), 0, s>>>(st.hist2, st.ctrl, Q, qs);
  SEG3D_LAUNCH_CHECK("seg3d_volume_stats_resolve");
  return SEG3D_OK;
}

template <int MC, bool VEC>
static void vs_moments_launch(dim3 grid, hipStream_t s, const float* volume, const unsigned char* sel, i64 nv, int M,
                              int mode, int clip, const VsState& st) {
  vs_moments_kernel<MC, VEC><<<grid, dim3(256), 0, s>>>(volume, sel, nv, M, mode, clip, st.ctrl, st.slots);
}

extern "C" int seg3d_volume_stats_accumulate_moments(const float* volume, const unsigned char* sel, long long voxels,
                                                     int M, int mode, int clip, void* state, void* stream) {
  VS_CHECK_STATE("seg3d_volume_stats_accumulate_moments");
  VS_CHECK_VOLUME("seg3d_volume_stats_accumulate_moments");
  const VsState st = vs_state(state, M);
  MC_DISPATCH(vs_moments_launch, M, mc_vec_rows(M, volume),
              (dim3(vs_grid_x(voxels, 256, 8, VS_MAX_GRID)), (hipStream_t)stream, volume, sel, (i64)voxels, M, mode, clip ? 1 : 0, st));
  SEG3D_LAUNCH_CHECK("seg3d_volume_stats_accumulate_moments");
  return SEG3D_OK;
}

extern "C" int seg3d_volume_stats_finish(void* state, int M, int Q, int clip, double* out, void* stream) {
  VS_CHECK_STATE("seg3d_volume_stats_finish");
  SEG3D_REQUIRE(out && ((uintptr_t)out & 7) == 0, "seg3d_volume_stats_finish: out must be an 8-byte aligned device buffer");
  SEG3D_REQUIRE(Q >= 0 && Q <= VS_MAXQ, "seg3d_volume_stats_finish: Q = %d order statistics, 0..4 are supported", Q);
  SEG3D_REQUIRE(!clip || Q >= 2, "seg3d_volume_stats_finish: the clamp needs the two order statistics q_0 <= q_1");
  const VsState st = vs_state(state, M);
  vs_finish_kernel<<<dim3(1), dim3(256), 0, (hipStream_t)stream>>>(st.ctrl, st.slots, M, Q, clip ? 1 : 0, out);
  SEG3D_LAUNCH_CHECK("seg3d_volume_stats_finish");
  return SEG3D_OK;
}

// the one-volume sequence: begin, three histogram + resolve levels (level 0 only when Q == 0), moments, finish
extern "C" int seg3d_volume_stats(const float* volume, const unsigned char* sel, long long voxels, int M, int mode, int Q,
                                  const double* quantiles, int clip, void* state, double* out, void* stream) {
  SEG3D_REQUIRE(Q >= 0 && Q <= VS_MAXQ, "seg3d_volume_stats: Q = %d order statistics, 0..4 are supported", Q);
  SEG3D_REQUIRE(!clip || (Q >= 2 && quantiles && quantiles[0] <= quantiles[1]),
                "seg3d_volume_stats: the clamp needs the two order statistics q_0 <= q_1");
  int rc = seg3d_volume_stats_begin(state, M, stream);
  for (int level = 0; rc == SEG3D_OK && level < (Q > 0 ? 3 : 1); ++level) {
    rc = seg3d_volume_stats_accumulate_hist(volume, sel, voxels, M, mode, level, state, stream);
    if (rc == SEG3D_OK) rc = seg3d_volume_stats_resolve(state, M, Q, quantiles, level, stream);
  }
  if (rc == SEG3D_OK) rc = seg3d_volume_stats_accumulate_moments(volume, sel, voxels, M, mode, clip, state, stream);
  if (rc == SEG3D_OK) rc = seg3d_volume_stats_finish(state, M, Q, clip, out, stream);
  return rc;
}
