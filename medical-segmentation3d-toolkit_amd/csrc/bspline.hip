// bspline.hip -- the cubic B-spline prefilter (the definition is stated in
// include/seg3d_hip.h): samples [Z][Y][X][M] -> coefficients of the same shape, whole-sample mirror, the three axes in turn
// (x, y, z).  Per line of n samples, with z = sqrt(3) - 2:
//   c+[0] = sum_{k < 24} z^k s[mirror(k)],  c+[i] = s[i] + z c+[i-1]          (causal, ascending)
//   c-[n-1] = z / (z^2 - 1) (c+[n-1] + z c+[n-2]),  c-[i] = z (c-[i+1] - c+[i]) (anti-causal, descending),  c = 6 c-
// One thread owns one line of one channel from end to end.  The running values c+ / c- (and the two values of the
// anti-causal start) are doubles in registers; c+ is parked as fp32 where c will stand and read back by the descending
// sweep, so a pass needs no workspace and may run in place.  The arithmetic of a line does not depend on M, on the tiling
// or on the alignment: channel m of an M-channel call equals the M = 1 call on plane m bit for bit, and two runs are
// bit-equal (no atomics, no cross-thread reduction).
//   y and z pass  bspline_axis_kernel: a thread per float column (x, m) [and z / y]; neighbouring lanes walk neighbouring
//                 floats, so every access of a wave is one contiguous 256-byte segment whatever M is -- the pass does not
//                 need the row width and has no <MC, VEC> instantiations.
//   x pass        bspline_x_kernel<MC, VEC>: the line runs along the contiguous axis, so a workgroup stages 256 / M lines
//                 x BSP_W positions through LDS (voxel rows moved as rows, mc_load_row / mc_store_row; the LDS image is
//                 transposed to [line, m][x] with an odd pitch: lane p reads word p * 63 + i, bank (i - p) mod 64, no
//                 conflict).  A line longer than a tile is walked tile by tile with the recurrence carried in registers
//                 (ascending, then descending): no halo, no approximation, and a workgroup only ever touches its own
//                 lines, so in place is safe.  The last tile of the ascending sweep stays in LDS for the descending one.
// All three passes are HBM streams: read s, write c+, read c+, write c per pass (the x pass of a line that fits one tile:
// read s, write c).
#include "seg3d_bspline.h"
#include "mc_device.h"
#include "seg3d_hip.h"

#define BSP_W 63       // x positions of an LDS tile = its pitch in floats (odd); 256 * 63 * 4 = 64512 bytes
#define BSP_BATCH 8    // loads in flight per thread of the strided passes

// c+[0] of a line: s(k) returns sample k (0 <= k < n) as double
template <typename Sample>
__device__ __forceinline__ double bspline_causal_init(int n, Sample s) {
  double acc = s(0), zk = SEG3D_BSPLINE_POLE;
  for (int k = 1; k < SEG3D_BSPLINE_HORIZON; ++k) {
    acc += zk * s(bspline_mirror(k, n));
    zk *= SEG3D_BSPLINE_POLE;
  }
  return acc;
}

// lines along an axis of n >= 2 samples and stride `inner` floats: column idx = (o, e), o < outer, e < inner, sample i at
// (o * n + i) * inner + e
__global__ __launch_bounds__(256) void bspline_axis_kernel(const float* src, float* dst, i64 outer, i64 inner, int n) {
  const i64 total = outer * inner;
  for (i64 idx = (i64)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (i64)gridDim.x * 256) {
    const i64 base = (idx / inner) * n * inner + idx % inner;
    const float* s = src + base;
    float* d = dst + base;
    double cp = bspline_causal_init(n, [&](int k) { return (double)s[k * inner]; });
    double prev = cp;
    d[0] = (float)cp;
    int i = 1;
    for (; i + BSP_BATCH <= n; i += BSP_BATCH) {
      float v[BSP_BATCH];
#pragma unroll
      for (int j = 0; j < BSP_BATCH; ++j) v[j] = s[(i + j) * inner];
#pragma unroll
      for (int j = 0; j < BSP_BATCH; ++j) {
        prev = cp;
        cp = (double)v[j] + SEG3D_BSPLINE_POLE * cp;
        d[(i + j) * inner] = (float)cp;
      }
    }
    for (; i < n; ++i) {
      prev = cp;
      cp = (double)s[i * inner] + SEG3D_BSPLINE_POLE * cp;
      d[i * inner] = (float)cp;
    }
    double cm = SEG3D_BSPLINE_LAST * (cp + SEG3D_BSPLINE_POLE * prev);
    d[(n - 1) * inner] = (float)(6.0 * cm);
    i = n - 2;
    for (; i - BSP_BATCH + 1 >= 0; i -= BSP_BATCH) {
      float v[BSP_BATCH];
#pragma unroll
      for (int j = 0; j < BSP_BATCH; ++j) v[j] = d[(i - j) * inner];
#pragma unroll
      for (int j = 0; j < BSP_BATCH; ++j) {
        cm = SEG3D_BSPLINE_POLE * (cm - (double)v[j]);
        d[(i - j) * inner] = (float)(6.0 * cm);
      }
    }
    for (; i >= 0; --i) {
      cm = SEG3D_BSPLINE_POLE * (cm - (double)d[i * inner]);
      d[i * inner] = (float)(6.0 * cm);
    }
  }
}

// positions [xs, xs + w) of lines [line0, line0 + nl) between memory (voxel rows of M floats) and the LDS image [l * M + m][x]
template <int MC, bool VEC>
__device__ __forceinline__ void bspline_tile_load(const float* p, float* tile, int M, int X, i64 line0, int nl, int xs, int w) {
  for (int r = threadIdx.x; r < nl * w; r += 256) {
    const int l = r / w, xi = r - l * w;
    float v[mc_regs<MC>];
    mc_load_row<MC, VEC>(p + ((line0 + l) * X + xs + xi) * M, v, M, 0.f);
#pragma unroll
    for (int m = 0; m < mc_regs<MC>; ++m)
      if (m < M) tile[(l * M + m) * BSP_W + xi] = v[m];
  }
}
template <int MC, bool VEC>
__device__ __forceinline__ void bspline_tile_store(float* p, const float* tile, int M, int X, i64 line0, int nl, int xs, int w) {
  for (int r = threadIdx.x; r < nl * w; r += 256) {
    const int l = r / w, xi = r - l * w;
    float v[mc_regs<MC>];
#pragma unroll
    for (int m = 0; m < mc_regs<MC>; ++m) v[m] = m < M ? tile[(l * M + m) * BSP_W + xi] : 0.f;
    mc_store_row<MC, VEC>(p + ((line0 + l) * X + xs + xi) * M, v, M);
  }
}

// lines along x, X >= 2: workgroup b owns lines [b * (256 / M), + 256 / M) of the Y * Z lines, thread p = l * M + m one of them
template <int MC, bool VEC>
__global__ __launch_bounds__(256) void bspline_x_kernel(const float* src, float* dst, int Mrt, int X, i64 nlines) {
  __shared__ float tile[256 * BSP_W];
  const int M = mc_width<MC>(Mrt);
  const int L = 256 / M;
  const i64 line0 = (i64)blockIdx.x * L;
  const int nl = (int)(nlines - line0 < L ? nlines - line0 : L);
  const bool active = (int)threadIdx.x < nl * M;
  float* mine = tile + threadIdx.x * BSP_W;
  const int nchunks = (X + BSP_W - 1) / BSP_W;
  double cp = 0.0, prev = 0.0, cm = 0.0;
  for (int c = 0; c < nchunks; ++c) {              // ascending: s -> c+
    const int xs = c * BSP_W, w = X - xs < BSP_W ? X - xs : BSP_W;
    bspline_tile_load<MC, VEC>(src, tile, M, X, line0, nl, xs, w);
    __syncthreads();
    if (active) {
      int i = 0;
      if (c == 0) {   // the 24 samples of the start lie in the first tile: X > 63 has mirror(k) = k, a shorter line is all here
        cp = bspline_causal_init(X, [&](int k) { return (double)mine[k]; });
        prev = cp;
        mine[0] = (float)cp;
        i = 1;
      }
      for (; i < w; ++i) {
        prev = cp;
        cp = (double)mine[i] + SEG3D_BSPLINE_POLE * cp;
        mine[i] = (float)cp;
      }
    }
    __syncthreads();
    if (c != nchunks - 1) {
      bspline_tile_store<MC, VEC>(dst, tile, M, X, line0, nl, xs, w);
      __syncthreads();
    }
  }
  for (int c = nchunks - 1; c >= 0; --c) {         // descending: c+ -> c
    const int xs = c * BSP_W, w = X - xs < BSP_W ? X - xs : BSP_W;
    if (c != nchunks - 1) {
      bspline_tile_load<MC, VEC>(dst, tile, M, X, line0, nl, xs, w);
      __syncthreads();
    }
    if (active) {
      int i = w - 1;
      if (c == nchunks - 1) {
        cm = SEG3D_BSPLINE_LAST * (cp + SEG3D_BSPLINE_POLE * prev);
        mine[i] = (float)(6.0 * cm);
        --i;
      }
      for (; i >= 0; --i) {
        cm = SEG3D_BSPLINE_POLE * (cm - (double)mine[i]);
        mine[i] = (float)(6.0 * cm);
      }
    }
    __syncthreads();
    bspline_tile_store<MC, VEC>(dst, tile, M, X, line0, nl, xs, w);
    __syncthreads();
  }
}

template <int MC, bool VEC>
static void bspline_x_launch(const float* src, float* dst, int M, int X, i64 nlines, hipStream_t s) {
  const int L = 256 / M;
  hipLaunchKernelGGL((bspline_x_kernel<MC, VEC>), dim3((unsigned)((nlines + L - 1) / L)), dim3(256), 0, s, src, dst, M, X,
                     nlines);
}

static void bspline_axis_launch(const float* src, float* dst, i64 outer, i64 inner, int n, hipStream_t s) {
  i64 blocks = (outer * inner + 255) / 256;
  if (blocks > (1ll << 20)) blocks = 1ll << 20;
  hipLaunchKernelGGL(bspline_axis_kernel, dim3((unsigned)blocks), dim3(256), 0, s, src, dst, outer, inner, n);
}

// src [Z][Y][X][M] samples -> dst coefficients, dst == src (in place) or disjoint; an axis of one voxel is left as it is
extern "C" int seg3d_bspline_prefilter_mc(const float* src, float* dst, int X, int Y, int Z, int M, void* stream) {
  SEG3D_REQUIRE(src && dst, "seg3d_bspline_prefilter_mc: null pointer");
  SEG3D_REQUIRE(M >= 1 && M <= 8, "seg3d_bspline_prefilter_mc: M = %d channels, 1..8 are supported", M);
  SEG3D_REQUIRE(X > 0 && Y > 0 && Z > 0, "seg3d_bspline_prefilter_mc: bad dims %d x %d x %d", X, Y, Z);
  SEG3D_REQUIRE((i64)Y * Z <= (i64)0x7fffffff * (256 / M), "seg3d_bspline_prefilter_mc: too many lines for one grid");
  hipStream_t s = (hipStream_t)stream;
  const float* in = src;
  if (X > 1) {
    MC_DISPATCH(bspline_x_launch, M, mc_vec_rows(M, src, dst), (in, dst, M, X, (i64)Y * Z, s));
    in = dst;
  }
  if (Y > 1) {
    bspline_axis_launch(in, dst, Z, (i64)X * M, Y, s);
    in = dst;
  }
  if (Z > 1) {
    bspline_axis_launch(in, dst, 1, (i64)Y * X * M, Z, s);
    in = dst;
  }
  if (in != dst && hipMemcpyAsync(dst, src, (size_t)X * Y * Z * M * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) {
    seg3d_set_error("seg3d_bspline_prefilter_mc: hipMemcpyAsync failed");
    return SEG3D_ERR_LAUNCH;
  }
  SEG3D_LAUNCH_CHECK("seg3d_bspline_prefilter_mc");
  return SEG3D_OK;
}
