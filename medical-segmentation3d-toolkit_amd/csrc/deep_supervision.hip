// deep_supervision.hip -- auxiliary segmentation heads of a deeply supervised decoder and the label pyramid they train on.
//
// No counterpart in the reference (its V-Net / VB-Net train on the full-resolution output only).  A head is what
// nn.Conv3d(Cin, C, 1) + nn.Softmax(dim=1) computes on a decoder feature (64 / 128 / 256 channels at 1/2, 1/4, 1/8 resolution):
//   p[n][c][s] = softmax_c( b[c] + sum_ci w[c][ci] x[n,s][ci] )
// Both directions are HBM-bound streaming passes over the widest tensor, x (Cin floats per voxel against C of output):
//   forward   reads x once, writes p;                 the logits live in registers only
//   backward  reads p, dp and x once, writes dx once; dw / db leave as one partial slab per workgroup, summed in a fixed
//             order in fp64 by the finalize launch (no atomics: a captured replay equals an eager run bit for bit)
// Work split: a voxel row is spread over a 16-lane group, lane j holding the NQ channel quads j, j + 16, .. (one 16-byte load
// each; 16 lanes x 16 B = a whole 256-byte row segment per instruction; NQ = 1, 2, 4 is a template parameter); a group walks VPI
// voxels per tile so that every weight quad read from LDS is used VPI times and NQ * VPI loads per lane are in flight.  The dot products end
// with a 4-step xor butterfly inside the group.  Weights and bias are staged in LDS once per workgroup (<= 8 KB + 32 B).
// The grids are persistent: a few workgroups per CU walk the tiles with a stride of gridDim.x.
#include "seg3d_common.h"
#include "seg3d_hip.h"

#define DS_MAX_CIN 256
#define DS_MAX_C 8
#define DS_GROUP 16                       // lanes per voxel
#define DS_GROUPS (256 / DS_GROUP)        // voxel groups per workgroup
#define DS_BWD_MAX_BLOCKS 1024            // bound of the backward grid = slabs of the workspace

__device__ __forceinline__ float ds_group_sum(float v) {
#pragma unroll
  for (int off = DS_GROUP / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, DS_GROUP);
  return v;   // in every lane of the group
}

__device__ __forceinline__ float ds_dot4(seg3d_f32x4 a, seg3d_f32x4 b, float acc) {
  acc = fmaf(a[0], b[0], acc);
  acc = fmaf(a[1], b[1], acc);
  acc = fmaf(a[2], b[2], acc);
  return fmaf(a[3], b[3], acc);
}

__device__ __forceinline__ void ds_stage_weights(const float* __restrict__ w, const float* __restrict__ b, float* w_s,
                                                 float* b_s, int Cin, int C) {
  for (int i = threadIdx.x; i < C * Cin / 4; i += 256)
    reinterpret_cast<seg3d_f32x4*>(w_s)[i] = reinterpret_cast<const seg3d_f32x4*>(w)[i];
  if (b_s && threadIdx.x < DS_MAX_C) b_s[threadIdx.x] = (b && (int)threadIdx.x < C) ? b[threadIdx.x] : 0.f;
  __syncthreads();
}

// ---- forward ------------------------------------------------------------------------------------------------------------
template <int C, int VPI, int NQ>
__global__ __launch_bounds__(256) void ds_head_fwd_kernel(const float* __restrict__ x, i64 ldx, const float* __restrict__ w,
                                                            const float* __restrict__ b, float* __restrict__ probs, i64 S,
                                                            i64 V, int Cin, i64 ntiles) {
  __shared__ __attribute__((aligned(16))) float w_s[DS_MAX_C * DS_MAX_CIN];
  __shared__ float b_s[DS_MAX_C];
  ds_stage_weights(w, b, w_s, b_s, Cin, C);
  const int g = threadIdx.x / DS_GROUP, j = threadIdx.x % DS_GROUP;
  const int nq = Cin / 4;
  for (i64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const i64 v0 = (tile * DS_GROUPS + g) * VPI;      // a wave's 4 groups own 4 * VPI consecutive voxels
    seg3d_f32x4 xr[VPI][NQ];
#pragma unroll
    for (int u = 0; u < VPI; ++u)
#pragma unroll
      for (int i = 0; i < NQ; ++i) {
        const int q = j + DS_GROUP * i;
        xr[u][i] = (q < nq && v0 + u < V) ? *reinterpret_cast<const seg3d_f32x4*>(x + (v0 + u) * ldx + 4 * q)
                                          : seg3d_f32x4{0.f, 0.f, 0.f, 0.f};
      }
    float acc[VPI][C];
#pragma unroll
    for (int u = 0; u < VPI; ++u)
#pragma unroll
      for (int c = 0; c < C; ++c) acc[u][c] = 0.f;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int q = j + DS_GROUP * i;
      if (q < nq) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const seg3d_f32x4 w4 = *reinterpret_cast<const seg3d_f32x4*>(w_s + c * Cin + 4 * q);
#pragma unroll
          for (int u = 0; u < VPI; ++u) acc[u][c] = ds_dot4(xr[u][i], w4, acc[u][c]);
        }
      }
    }
    // lane j < VPI of the group finishes voxel v0 + j
    float l[C];
#pragma unroll
    for (int c = 0; c < C; ++c) l[c] = 0.f;
#pragma unroll
    for (int u = 0; u < VPI; ++u)
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float t = ds_group_sum(acc[u][c]);
        if (j == u) l[c] = t;
      }
    const i64 v = v0 + j;
    if (j < VPI && v < V) {
      float mx = -INFINITY;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        l[c] += b_s[c];
        mx = fmaxf(mx, l[c]);
      }
      float sum = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        l[c] = expf(l[c] - mx);
        sum += l[c];
      }
      const i64 n = v / S, s = v - n * S;
#pragma unroll
      for (int c = 0; c < C; ++c) probs[(n * C + c) * S + s] = l[c] / sum;
    }
  }
}

// ---- backward -----------------------------------------------------------------------------------------------------------
// part[block][C * Cin + C]: the block's sums of g_c x[ci] (C rows of Cin) and of g_c
template <int C, int VPI, int NQ>
__global__ __launch_bounds__(256) void ds_head_bwd_kernel(const float* __restrict__ probs, const float* __restrict__ dprobs,
                                                            const float* __restrict__ x, i64 ldx, const float* __restrict__ w,
                                                            float* __restrict__ dx, i64 ld_dx, float* __restrict__ part, i64 S,
                                                            i64 V, int Cin, i64 ntiles) {
  __shared__ __attribute__((aligned(16))) float w_s[DS_MAX_C * DS_MAX_CIN];   // weights; the slab reduction re-uses it at the end
  __shared__ float db_s[4][DS_MAX_C];
  ds_stage_weights(w, nullptr, w_s, nullptr, Cin, C);
  const int g = threadIdx.x / DS_GROUP, j = threadIdx.x % DS_GROUP;
  const int nq = Cin / 4;
  seg3d_f32x4 dwr[C][NQ];
  float dbr[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    dbr[c] = 0.f;
#pragma unroll
    for (int i = 0; i < NQ; ++i) dwr[c][i] = seg3d_f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (i64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const i64 v0 = (tile * DS_GROUPS + g) * VPI;
    seg3d_f32x4 xr[VPI][NQ];
#pragma unroll
    for (int u = 0; u < VPI; ++u)
#pragma unroll
      for (int i = 0; i < NQ; ++i) {
        const int q = j + DS_GROUP * i;
        xr[u][i] = (q < nq && v0 + u < V) ? *reinterpret_cast<const seg3d_f32x4*>(x + (v0 + u) * ldx + 4 * q)
                                          : seg3d_f32x4{0.f, 0.f, 0.f, 0.f};
      }
    // lane j < VPI: softmax backward of voxel v0 + j (zeros past the end), then handed to the whole group
    float gl[C];
#pragma unroll
    for (int c = 0; c < C; ++c) gl[c] = 0.f;
    const i64 v = v0 + j;
    if (j < VPI && v < V) {
      const i64 n = v / S, s = v - n * S;
      float p[C], d[C], dot = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        p[c] = probs[(n * C + c) * S + s];
        d[c] = dprobs[(n * C + c) * S + s];
        dot = fmaf(p[c], d[c], dot);
      }
#pragma unroll
      for (int c = 0; c < C; ++c) {
        gl[c] = p[c] * (d[c] - dot);
        dbr[c] += gl[c];
      }
    }
    float gv[VPI][C];
#pragma unroll
    for (int u = 0; u < VPI; ++u)
#pragma unroll
      for (int c = 0; c < C; ++c) gv[u][c] = __shfl(gl[c], u, DS_GROUP);
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int q = j + DS_GROUP * i;
      if (q < nq) {
        seg3d_f32x4 o[VPI];
#pragma unroll
        for (int u = 0; u < VPI; ++u) o[u] = seg3d_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const seg3d_f32x4 w4 = *reinterpret_cast<const seg3d_f32x4*>(w_s + c * Cin + 4 * q);
#pragma unroll
          for (int u = 0; u < VPI; ++u)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              o[u][k] = fmaf(gv[u][c], w4[k], o[u][k]);
              dwr[c][i][k] = fmaf(gv[u][c], xr[u][i][k], dwr[c][i][k]);
            }
        }
#pragma unroll
        for (int u = 0; u < VPI; ++u)
          if (v0 + u < V) *reinterpret_cast<seg3d_f32x4*>(dx + (v0 + u) * ld_dx + 4 * q) = o[u];
      }
    }
  }
  // the workgroup's slab: the 4 groups of a wave by shuffles, the 4 waves one after the other through LDS (fixed order)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int c = 0; c < C; ++c) {
#pragma unroll
    for (int i = 0; i < NQ; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float t = dwr[c][i][k];
        t += __shfl_xor(t, 16, 64);
        t += __shfl_xor(t, 32, 64);
        dwr[c][i][k] = t;
      }
    // db: lanes j < VPI of every group hold a share; the other lanes hold 0
    dbr[c] = wave_sum(dbr[c]);
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < C; ++c) db_s[wave][c] = dbr[c];
  }
  for (int wv = 0; wv < 4; ++wv) {
    __syncthreads();        // (first round: every wave is done reading the weights)
    if (wave == wv && lane < DS_GROUP) {
#pragma unroll
      for (int i = 0; i < NQ; ++i) {
        const int q = lane + DS_GROUP * i;
        if (q < nq) {
#pragma unroll
          for (int c = 0; c < C; ++c) {
            seg3d_f32x4* dst = reinterpret_cast<seg3d_f32x4*>(w_s + c * Cin + 4 * q);
            seg3d_f32x4 t = dwr[c][i];
            if (wv) {
              const seg3d_f32x4 o = *dst;
#pragma unroll
              for (int k = 0; k < 4; ++k) t[k] = o[k] + t[k];
            }
            *dst = t;
          }
        }
      }
    }
  }
  __syncthreads();
  float* slab = part + (i64)blockIdx.x * (C * Cin + C);
  for (int i = threadIdx.x; i < C * Cin; i += 256) slab[i] = w_s[i];
  if (threadIdx.x < C) {
    const int c = threadIdx.x;
    slab[C * Cin + c] = ((db_s[0][c] + db_s[1][c]) + db_s[2][c]) + db_s[3][c];
  }
}

// out[k] (+)= sum over the slabs of part[slab][k], k < K = C * Cin + C; the first C * Cin go to dw, the rest to db.
// 16 outputs per workgroup, 16 lanes stride over the slabs of each in fp64, then one thread adds the 16 shares in order.
__global__ __launch_bounds__(256) void ds_head_bwd_finalize_kernel(const float* __restrict__ part, float* __restrict__ dw,
                                                                     float* __restrict__ db, int nslab, int K, int nw,
                                                                     int accumulate) {
  __shared__ double red[16][17];
  const int kl = threadIdx.x & 15, bl = threadIdx.x >> 4;
  const int k = blockIdx.x * 16 + kl;
  double acc = 0.0;
  if (k < K)
    for (int s = bl; s < nslab; s += 16) acc += (double)part[(i64)s * K + k];
  red[bl][kl] = acc;
  __syncthreads();
  if (bl == 0 && k < K) {
    double t = 0.0;
    for (int r = 0; r < 16; ++r) t += red[r][kl];
    if (k < nw) {
      if (dw) dw[k] = (accumulate & 1) ? dw[k] + (float)t : (float)t;
    } else if (db) {
      db[k - nw] = (accumulate & 2) ? db[k - nw] + (float)t : (float)t;
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
// Kernels are instantiated per class count C and per NQ = channel quads a lane holds (1, 2 or 4: Cin <= 64, <= 128, <= 256), so
// the register arrays are as large as the shape needs and no larger; VPI, the voxels a group has in flight, is chosen so that
// the loads in flight stay at 8 - 16 per lane forward, and so that the backward's dw accumulators (C x NQ quads per lane) leave
// room for them.
constexpr int ds_nq(int Cin) { return Cin <= 64 ? 1 : (Cin <= 128 ? 2 : 4); }
constexpr int ds_fwd_vpi(int NQ) { return NQ == 1 ? 8 : 4; }
constexpr int ds_bwd_vpi(int C, int NQ) { return C * NQ <= 4 ? 8 : (C * NQ <= 8 ? 4 : (C * NQ <= 16 ? 2 : 1)); }
static inline i64 ds_tiles(i64 V, int vpi) { return (V + (i64)DS_GROUPS * vpi - 1) / ((i64)DS_GROUPS * vpi); }
static inline i64 ds_bwd_slabs(i64 V, int Cin, int C) {      // pure function of the shape: sizes the workspace
  const i64 t = ds_tiles(V, ds_bwd_vpi(C, ds_nq(Cin)));
  return t < DS_BWD_MAX_BLOCKS ? t : DS_BWD_MAX_BLOCKS;
}
static inline unsigned ds_bwd_grid(i64 V, int Cin, int C) {  // the grid actually launched (and summed by the finalize): <= the slabs
  const i64 slabs = ds_bwd_slabs(V, Cin, C), want = (i64)seg3d_device_cus() * 4;
  return (unsigned)(slabs < want ? slabs : want);
}

extern "C" int seg3d_ds_head_supported(int Cin, int C) {
  return Cin >= 4 && Cin % 4 == 0 && Cin <= DS_MAX_CIN && C >= 1 && C <= DS_MAX_C;
}

static int ds_check(const char* name, const float* x, int ldx, int N, i64 S, int Cin, int C) {
  if (!seg3d_ds_head_supported(Cin, C))
    SEG3D_UNSUPPORTED("%s: needs Cin %% 4 == 0, Cin <= %d and 1 <= C <= %d (got Cin = %d, C = %d)", name, DS_MAX_CIN, DS_MAX_C,
                      Cin, C);
  SEG3D_REQUIRE(N > 0 && S > 0, "%s: bad shape N = %d, S = %lld", name, N, (long long)S);
  SEG3D_REQUIRE(ldx == 0 || (ldx >= Cin && ldx % 4 == 0), "%s: row stride %d must be 0 or a multiple of 4 that is >= Cin = %d",
                name, ldx, Cin);
  SEG3D_REQUIRE(((uintptr_t)x & 15) == 0, "%s: rows must be 16-byte aligned", name);
  return SEG3D_OK;
}

#define DS_DISPATCH_NQ(CC, NQ, LAUNCH)                                                                   \
  switch (NQ) {                                                                                          \
    case 1: LAUNCH(CC, 1); break;                                                                        \
    case 2: LAUNCH(CC, 2); break;                                                                        \
    default: LAUNCH(CC, 4); break;                                                                       \
  }
#define DS_DISPATCH(C, NQ, LAUNCH)                                                                       \
  switch (C) {                                                                                           \
    case 1: DS_DISPATCH_NQ(1, NQ, LAUNCH) break;                                                         \
    case 2: DS_DISPATCH_NQ(2, NQ, LAUNCH) break;                                                         \
    case 3: DS_DISPATCH_NQ(3, NQ, LAUNCH) break;                                                         \
    case 4: DS_DISPATCH_NQ(4, NQ, LAUNCH) break;                                                         \
    case 5: DS_DISPATCH_NQ(5, NQ, LAUNCH) break;                                                         \
    case 6: DS_DISPATCH_NQ(6, NQ, LAUNCH) break;                                                         \
    case 7: DS_DISPATCH_NQ(7, NQ, LAUNCH) break;                                                         \
    default: DS_DISPATCH_NQ(8, NQ, LAUNCH) break;                                                        \
  }

extern "C" int seg3d_ds_head_fwd(const float* x, int ldx, const float* w, const float* b, float* probs, int N, long long S,
                                 int Cin, int C, void* stream) {
  SEG3D_REQUIRE(x && w && probs, "seg3d_ds_head_fwd: null pointer");
  const int rc = ds_check("seg3d_ds_head_fwd", x, ldx, N, S, Cin, C);
  if (rc != SEG3D_OK) return rc;
  SEG3D_REQUIRE(((uintptr_t)w & 15) == 0, "seg3d_ds_head_fwd: the weight must be 16-byte aligned");
  const i64 V = (i64)N * S;
  const i64 want = (i64)seg3d_device_cus() * 8;
  const i64 ld = ldx ? ldx : Cin;
  const int nq = ds_nq(Cin);
#define DS_FWD(CC, QQ)                                                                                                        \
  {                                                                                                                           \
    constexpr int vpi = ds_fwd_vpi(QQ);                                                                                       \
    const i64 ntiles = ds_tiles(V, vpi);                                                                                      \
    hipLaunchKernelGGL((ds_head_fwd_kernel<CC, vpi, QQ>), dim3((unsigned)(ntiles < want ? ntiles : want)), dim3(256), 0,      \
                       (hipStream_t)stream, x, ld, w, b, probs, (i64)S, V, Cin, ntiles);                                      \
  }
  DS_DISPATCH(C, nq, DS_FWD)
#undef DS_FWD
  SEG3D_LAUNCH_CHECK("seg3d_ds_head_fwd");
  return SEG3D_OK;
}

extern "C" long long seg3d_ds_head_bwd_workspace_floats(int N, long long S, int Cin, int C) {
  if (!seg3d_ds_head_supported(Cin, C) || N <= 0 || S <= 0) return 0;
  return ds_bwd_slabs((i64)N * S, Cin, C) * ((i64)C * Cin + C);
}

extern "C" int seg3d_ds_head_bwd(const float* probs, const float* dprobs, const float* x, int ldx, const float* w, float* dx,
                                 int ld_dx, float* workspace, int N, long long S, int Cin, int C, void* stream) {
  SEG3D_REQUIRE(probs && dprobs && x && w && dx && workspace, "seg3d_ds_head_bwd: null pointer");
  const int rc = ds_check("seg3d_ds_head_bwd", x, ldx, N, S, Cin, C);
  if (rc != SEG3D_OK) return rc;
  SEG3D_REQUIRE(ld_dx == 0 || (ld_dx >= Cin && ld_dx % 4 == 0),
                "seg3d_ds_head_bwd: dx row stride %d must be 0 or a multiple of 4 that is >= Cin = %d", ld_dx, Cin);
  SEG3D_REQUIRE(((uintptr_t)w & 15) == 0 && ((uintptr_t)dx & 15) == 0, "seg3d_ds_head_bwd: w and dx must be 16-byte aligned");
  const i64 V = (i64)N * S;
  const unsigned grid = ds_bwd_grid(V, Cin, C);
  const i64 ld = ldx ? ldx : Cin, ldd = ld_dx ? ld_dx : Cin;
  const int nq = ds_nq(Cin);
#define DS_BWD(CC, QQ)                                                                                                          \
  {                                                                                                                             \
    constexpr int vpi = ds_bwd_vpi(CC, QQ);                                                                                     \
    hipLaunchKernelGGL((ds_head_bwd_kernel<CC, vpi, QQ>), dim3(grid), dim3(256), 0, (hipStream_t)stream, probs, dprobs, x, ld, w, \
                       dx, ldd, workspace, (i64)S, V, Cin, ds_tiles(V, vpi));                                                   \
  }
  DS_DISPATCH(C, nq, DS_BWD)
#undef DS_BWD
  SEG3D_LAUNCH_CHECK("seg3d_ds_head_bwd");
  return SEG3D_OK;
}

extern "C" int seg3d_ds_head_bwd_finalize(const float* workspace, float* dw, float* db, int N, long long S, int Cin, int C,
                                          int accumulate, void* stream) {
  SEG3D_REQUIRE(workspace && (dw || db), "seg3d_ds_head_bwd_finalize: null pointer");
  if (!seg3d_ds_head_supported(Cin, C))
    SEG3D_UNSUPPORTED("seg3d_ds_head_bwd_finalize: unsupported head Cin = %d, C = %d", Cin, C);
  SEG3D_REQUIRE(N > 0 && S > 0 && (accumulate & ~3) == 0, "seg3d_ds_head_bwd_finalize: bad arguments");
  const int K = C * Cin + C;
  hipLaunchKernelGGL(ds_head_bwd_finalize_kernel, dim3((K + 15) / 16), dim3(256), 0, (hipStream_t)stream, workspace, dw, db,
                     (int)ds_bwd_grid((i64)N * S, Cin, C), K, C * Cin, accumulate);
  SEG3D_LAUNCH_CHECK("seg3d_ds_head_bwd_finalize");
  return SEG3D_OK;
}

// ---- label pyramid ------------------------------------------------------------------------------------------------------
struct DsPyramid {
  float* out[3];
  i64 end[3];      // running end of level k's elements in the combined index space
};

__global__ __launch_bounds__(256) void label_pyramid_kernel(const float* __restrict__ mask, DsPyramid pyr, int levels, int D, int H,
                                                              int W) {
  const i64 total = pyr.end[levels - 1];
  for (i64 idx = (i64)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (i64)gridDim.x * 256) {
    int k = 0;
    i64 e = idx;
    if (levels > 1 && idx >= pyr.end[0]) { k = 1; e = idx - pyr.end[0]; }
    if (levels > 2 && idx >= pyr.end[1]) { k = 2; e = idx - pyr.end[1]; }
    const int f = 2 << k;
    const int Wk = W / f, Hk = H / f, Dk = D / f;
    const int xo = (int)(e % Wk);
    i64 r = e / Wk;
    const int yo = (int)(r % Hk);
    r /= Hk;
    const int zo = (int)(r % Dk);
    const i64 n = r / Dk;
    pyr.out[k][e] = mask[((n * D + (i64)zo * f) * H + (i64)yo * f) * W + (i64)xo * f];
  }
}

extern "C" int seg3d_label_pyramid(const float* mask, float* out1, float* out2, float* out3, int N, int D, int H, int W,
                                   int levels, void* stream) {
  SEG3D_REQUIRE(mask && N > 0 && D > 0 && H > 0 && W > 0, "seg3d_label_pyramid: bad arguments");
  SEG3D_REQUIRE(levels >= 1 && levels <= 3, "seg3d_label_pyramid: levels %d not in [1, 3]", levels);
  const int f = 1 << levels;
  SEG3D_REQUIRE(D % f == 0 && H % f == 0 && W % f == 0, "seg3d_label_pyramid: size (%d, %d, %d) is not divisible by %d", D, H, W,
                f);
  DsPyramid pyr;
  float* outs[3] = {out1, out2, out3};
  i64 end = 0;
  for (int k = 0; k < 3; ++k) {
    pyr.out[k] = outs[k];
    if (k < levels) {
      SEG3D_REQUIRE(outs[k], "seg3d_label_pyramid: output %d is null", k + 1);
      const int fk = 2 << k;
      end += (i64)N * (D / fk) * (H / fk) * (W / fk);
    }
    pyr.end[k] = end;
  }
  hipLaunchKernelGGL(label_pyramid_kernel, dim3(seg3d_ew_grid(end, 256)), dim3(256), 0, (hipStream_t)stream, mask, pyr, levels, D,
                     H, W);
  SEG3D_LAUNCH_CHECK("seg3d_label_pyramid");
  return SEG3D_OK;
}
