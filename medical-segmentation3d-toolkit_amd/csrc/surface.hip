// surface.hip -- surface-distance evaluation metrics (HD, HD95, ASSD).
//
// For one label: A = (gt == l), B = (seg == l) on a [Z][Y][X] grid with spacing (sx, sy, sz).
//   surface dA = voxels of A with a 6-neighbour outside A (outside the volume counts as outside A)
//   d(p, dB)  = Euclidean distance in physical units from voxel centre p to the nearest dB voxel centre
// The metrics need d(p, dB) for p in dA and d(q, dA) for q in dB.  Here:
//   seg3d_label_surface      one pass over a label volume (any of the five label dtypes): the surface mask, the
//                            number of surface voxels and the bounding box of the surface voxels (shared by dA and dB)
//   seg3d_surface_distance   exact separable squared EDT to the feature surface (Meijster's lower envelope) restricted
//                            to that box -- every feature and every query voxel lies inside it, so the restriction is
//                            exact -- in three passes:
//                              x: one wave per row, max/min scans give the 1-D voxel distance g (int32)
//                              y: one thread per (z, x) column, lanes on consecutive x (coalesced), envelope of
//                                 sx^2 g^2 along y -> f2 (fp64)
//                              z: one thread per (y, x) column, same envelope along z; the back scan emits the squared
//                                 distance only at query voxels, compacted into the caller's buffer, and reduces
//                                 (count, max, fp64 sum of distances) per workgroup; a one-block finalize adds the
//                                 partials in a fixed order, so the statistics are bit-reproducible
// All envelope arithmetic is fp64.  For unit spacing every value is an integer far below 2^53 and the floor of a
// correctly rounded quotient of two such integers is the exact floor, so the squared distances are exact.
// The box is read on the device: grids are sized from (X, Y, Z) alone, nothing synchronises or allocates, and the
// launches can be captured.
#include "label_device.h"
#include "seg3d_hip.h"

#define SURF_BLOCK 256
#define SURF_MAX_BLOCKS 4096
#define SURF_CHUNK 8   // loads issued back to back ahead of the serial envelope scan

static inline i64 surf_align(i64 b) { return (b + 255) & ~(i64)255; }

struct SurfBox {
  int x0, y0, z0, xb, yb, zb;   // origin and extent; extent 0 when the box is empty
};

// clamped to the volume, so a box that the caller got wrong cannot send a pass outside its buffers
__device__ __forceinline__ SurfBox surf_load_box(const int* box, int X, int Y, int Z) {
  SurfBox b;
  b.x0 = max(box[0], 0); b.y0 = max(box[1], 0); b.z0 = max(box[2], 0);
  const int x1 = min(box[3], X - 1), y1 = min(box[4], Y - 1), z1 = min(box[5], Z - 1);
  const bool empty = x1 < b.x0 || y1 < b.y0 || z1 < b.z0;
  b.xb = empty ? 0 : x1 - b.x0 + 1;
  b.yb = empty ? 0 : y1 - b.y0 + 1;
  b.zb = empty ? 0 : z1 - b.z0 + 1;
  return b;
}

// ---- surface extraction -------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(SURF_BLOCK) void label_surface_kernel(const T* __restrict__ vol, int X, int Y, int Z, T l,
                                                                   unsigned char* __restrict__ surf, int* __restrict__ box,
                                                                   int* __restrict__ count) {
  const unsigned XY = (unsigned)X * (unsigned)Y, n = XY * (unsigned)Z;
  int cnt = 0;
  LabelBox bx;
  for (unsigned i = blockIdx.x * SURF_BLOCK + threadIdx.x; i < n; i += gridDim.x * SURF_BLOCK) {
    const int x = (int)(i % (unsigned)X), y = (int)((i / (unsigned)X) % (unsigned)Y), z = (int)(i / XY);
    bool s = false;
    if (vol[i] == l) {
      const bool inner = x > 0 && x < X - 1 && y > 0 && y < Y - 1 && z > 0 && z < Z - 1 && vol[i - 1] == l &&
                         vol[i + 1] == l && vol[i - X] == l && vol[i + X] == l && vol[i - XY] == l && vol[i + XY] == l;
      s = !inner;
    }
    surf[i] = s ? 1 : 0;
    if (s) {
      ++cnt;
      bx.add(x, y, z);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
  if ((threadIdx.x & 63) == 0 && cnt > 0) atomicAdd(count, cnt);   // like the box: per wave that found surface voxels
  bx.wave_commit(box);
}

extern "C" int seg3d_label_surface(const void* labels, int dtype, int X, int Y, int Z, int label, unsigned char* surface,
                                   int* box_device, int* count_device, void* stream) {
  SEG3D_REQUIRE(labels && surface && box_device && count_device, "seg3d_label_surface: null pointer");
  SEG3D_REQUIRE(X > 0 && Y > 0 && Z > 0 && (i64)X * Y * Z < (1ll << 31),
                "seg3d_label_surface: bad volume size %d x %d x %d (1 .. 2^31 - 1 voxels)", X, Y, Z);
  const int rc = label_dispatch(dtype, "seg3d_label_surface", [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((label_surface_kernel<T>), dim3(seg3d_ew_grid((i64)X * Y * Z, SURF_BLOCK)), dim3(SURF_BLOCK), 0,
                       (hipStream_t)stream, (const T*)labels, X, Y, Z, (T)label, surface, box_device, count_device);
  });
  if (rc != SEG3D_OK) return rc;
  SEG3D_LAUNCH_CHECK("seg3d_label_surface");
  return SEG3D_OK;
}

// ---- pass x: 1-D voxel distance to the nearest feature of the row (-1: none) ---------------------------------------
// One wave per box row, 64 consecutive x per step: an inclusive max-scan of (feature ? x : -1) from the left, then a
// min-scan of (feature ? x : INT_MAX) from the right.  g[(z * yb + y) * xb + x] in box coordinates.
__global__ __launch_bounds__(SURF_BLOCK) void edt_rows_kernel(const unsigned char* __restrict__ feat, const int* __restrict__ box,
                                                              int X, int Y, int Z, int* __restrict__ g) {
  const SurfBox b = surf_load_box(box, X, Y, Z);
  const int lane = threadIdx.x & 63;
  const i64 rows = (i64)b.yb * b.zb;
  for (i64 r = (i64)blockIdx.x * (SURF_BLOCK / 64) + (threadIdx.x >> 6); r < rows; r += (i64)gridDim.x * (SURF_BLOCK / 64)) {
    const int y = (int)(r % b.yb), z = (int)(r / b.yb);
    const unsigned char* row = feat + ((i64)(b.z0 + z) * Y + (b.y0 + y)) * X + b.x0;
    int* out = g + r * b.xb;
    int last = -1;
    for (int xs = 0; xs < b.xb; xs += 64) {
      const int x = xs + lane;
      int v = (x < b.xb && row[x]) ? x : -1;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int u = __shfl_up(v, off, 64);
        if (lane >= off) v = max(v, u);
      }
      v = max(v, last);
      if (x < b.xb) out[x] = v >= 0 ? x - v : -1;
      last = __shfl(v, 63, 64);
    }
    int next = INT_MAX;
    for (int xs = ((b.xb - 1) / 64) * 64; xs >= 0; xs -= 64) {
      const int x = xs + lane;
      int v = (x < b.xb && row[x]) ? x : INT_MAX;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int u = __shfl_down(v, off, 64);
        if (lane + off < 64) v = min(v, u);
      }
      v = min(v, next);
      if (x < b.xb) {
        const int gl = out[x], gr = v != INT_MAX ? v - x : -1;
        out[x] = gl < 0 ? gr : (gr < 0 ? gl : min(gl, gr));
      }
      next = __shfl(v, 0, 64);
    }
  }
}

// ---- passes y and z: Meijster's lower envelope along one column ------------------------------------------------------
// Column c holds L samples f(u) (u = 0 .. L-1, missing = no feature); out(u) = min_i f(i) + w2 (u - i)^2.
// The stack of envelope entries (position s, start t, value fs) lives in the workspace at [k * ncols + c] (lanes on
// consecutive columns touch consecutive words when their stacks are equally deep); its top stays in registers.
struct EnvStack {
  int* s;
  int* t;
  double* f;
  i64 ncols, c;
  int q, sq, tq;
  double fq;
  __device__ __forceinline__ void push(int s_, int t_, double f_) {
    ++q;
    sq = s_; tq = t_; fq = f_;
    const i64 k = (i64)q * ncols + c;
    s[k] = s_; t[k] = t_; f[k] = f_;
  }
  __device__ __forceinline__ void pop() {
    if (--q >= 0) {
      const i64 k = (i64)q * ncols + c;
      sq = s[k]; tq = t[k]; fq = f[k];
    }
  }
};

__device__ __forceinline__ double env_f(int u, int s, double fs, double w2) {
  const double d = (double)(u - s);
  return fs + w2 * (d * d);
}

// forward scan step: feature u with value fu joins the envelope
__device__ __forceinline__ void env_add(EnvStack& st, int u, double fu, double w2, int L) {
  while (st.q >= 0 && env_f(st.tq, st.sq, st.fq, w2) > env_f(st.tq, u, fu, w2)) st.pop();
  if (st.q < 0) {
    st.push(u, 0, fu);
  } else {
    // Sep(s, u) = floor((fu - fs + w2 (u^2 - s^2)) / (2 w2 (u - s)))
    const double du = (double)(u - st.sq), su = (double)((i64)u + st.sq);
    // not popped means the intersection lies at or beyond t[q]; keep the starts strictly increasing should rounding say
    // otherwise (only possible for non-integer spacing, and then only at a tie)
    const double w = fmax(1.0 + floor((fu - st.fq + w2 * (du * su)) / (2.0 * w2 * du)), (double)st.tq + 1.0);
    if (w < (double)L) st.push(u, (int)w, fu);
  }
}

// pass y: columns (z, x) of the box, input g (x distances, voxels), output f2 = squared distance in the (x, y) plane
__global__ __launch_bounds__(SURF_BLOCK) void edt_cols_y_kernel(const int* __restrict__ g, const int* __restrict__ box,
                                                                int X, int Y, int Z, double wx2, double wy2, int* __restrict__ st_s,
                                                                int* __restrict__ st_t, double* __restrict__ st_f,
                                                                double* __restrict__ f2) {
  const SurfBox b = surf_load_box(box, X, Y, Z);
  const i64 ncols = (i64)b.zb * b.xb, step = (i64)b.xb;
  const int L = b.yb;
  for (i64 c = (i64)blockIdx.x * SURF_BLOCK + threadIdx.x; c < ncols; c += (i64)gridDim.x * SURF_BLOCK) {
    const i64 base = (c / b.xb) * ((i64)b.yb * b.xb) + c % b.xb;
    EnvStack st{st_s, st_t, st_f, ncols, c, -1, 0, 0, 0.0};
    for (int u0 = 0; u0 < L; u0 += SURF_CHUNK) {
      int v[SURF_CHUNK];
#pragma unroll
      for (int j = 0; j < SURF_CHUNK; ++j) v[j] = u0 + j < L ? g[base + (i64)(u0 + j) * step] : -1;
#pragma unroll
      for (int j = 0; j < SURF_CHUNK; ++j)
        if (v[j] >= 0) env_add(st, u0 + j, wx2 * ((double)v[j] * (double)v[j]), wy2, L);
    }
    const double inf = __builtin_huge_val();
    for (int u = L - 1; u >= 0; --u) {   // the entry that covers u is the top one with t <= u (t[0] = 0)
      while (st.q > 0 && st.tq > u) st.pop();
      f2[base + (i64)u * step] = st.q >= 0 ? env_f(u, st.sq, st.fq, wy2) : inf;
    }
  }
}

// (count, max, sum) over the workgroup in a fixed order: the wave tree, then waves 0 .. 3 one after the other from zero.
// The result is valid in thread 0.
__device__ __forceinline__ void surf_stats_block_reduce(double& count, double& mx, double& sum,
                                                        double (&red)[SURF_BLOCK / 64][3]) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    count += __shfl_down(count, off, 64);
    mx = fmax(mx, __shfl_down(mx, off, 64));
    sum += __shfl_down(sum, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    const int wave = threadIdx.x >> 6;
    red[wave][0] = count;
    red[wave][1] = mx;
    red[wave][2] = sum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    count = mx = sum = 0.0;
    for (int w = 0; w < SURF_BLOCK / 64; ++w) {
      count += red[w][0];
      mx = fmax(mx, red[w][1]);
      sum += red[w][2];
    }
  }
}

// pass z: columns (y, x) of the box, input f2, emits the squared distance at every query voxel of the column
__global__ __launch_bounds__(SURF_BLOCK) void edt_cols_z_query_kernel(
    const double* __restrict__ f2, const unsigned char* __restrict__ query, const int* __restrict__ box, int X, int Y, int Z,
    double wz2, int* __restrict__ st_s, int* __restrict__ st_t, double* __restrict__ st_f, int* __restrict__ counter,
    double* __restrict__ dist2, int* __restrict__ index, i64 capacity, double* __restrict__ partials) {
  const SurfBox b = surf_load_box(box, X, Y, Z);
  const i64 ncols = (i64)b.yb * b.xb, step = ncols;
  const int L = b.zb, lane = threadIdx.x & 63;
  const i64 XY = (i64)X * Y;
  int cnt = 0;
  double mx = 0.0, sum = 0.0;
  for (i64 c = (i64)blockIdx.x * SURF_BLOCK + threadIdx.x; c < ncols; c += (i64)gridDim.x * SURF_BLOCK) {
    EnvStack st{st_s, st_t, st_f, ncols, c, -1, 0, 0, 0.0};
    for (int u0 = 0; u0 < L; u0 += SURF_CHUNK) {
      double v[SURF_CHUNK];
#pragma unroll
      for (int j = 0; j < SURF_CHUNK; ++j) v[j] = u0 + j < L ? f2[c + (i64)(u0 + j) * step] : __builtin_huge_val();
#pragma unroll
      for (int j = 0; j < SURF_CHUNK; ++j)
        if (v[j] < __builtin_huge_val()) env_add(st, u0 + j, v[j], wz2, L);
    }
    const int y = (int)(c / b.xb), x = (int)(c % b.xb);
    const i64 qcol = (i64)(b.y0 + y) * X + (b.x0 + x) + (i64)b.z0 * XY;   // query voxel (x, y, z0) of the volume
    for (int u = L - 1; u >= 0; --u) {
      const i64 vox = qcol + (i64)u * XY;
      const bool emit = query[vox] != 0;
      while (st.q > 0 && st.tq > u) st.pop();
      const double d2 = st.q >= 0 ? env_f(u, st.sq, st.fq, wz2) : __builtin_huge_val();
      const unsigned long long m = __ballot(emit);
      if (m) {
        const int leader = __ffsll((unsigned long long)m) - 1;
        int slot0 = 0;
        if (lane == leader) slot0 = atomicAdd(counter, (int)__popcll(m));
        slot0 = __shfl(slot0, leader, 64);
        if (emit) {
          const i64 slot = (i64)slot0 + __popcll(m & ((1ull << lane) - 1ull));
          if (slot < capacity) {
            dist2[slot] = d2;
            if (index) index[slot] = (int)vox;
          }
          ++cnt;
          mx = fmax(mx, d2);
          sum += sqrt(d2);
        }
      }
    }
  }
  // partials[blockIdx.x] = (count, max d^2, sum d)
  __shared__ double red[SURF_BLOCK / 64][3];
  double c = (double)cnt;
  surf_stats_block_reduce(c, mx, sum, red);
  if (threadIdx.x == 0) {
    partials[3 * blockIdx.x] = c;
    partials[3 * blockIdx.x + 1] = mx;
    partials[3 * blockIdx.x + 2] = sum;
  }
}

// stats = (count, max distance, sum of distances) from the per-workgroup partials, in a fixed order
__global__ __launch_bounds__(SURF_BLOCK) void surface_stats_finalize_kernel(const double* __restrict__ partials, int nparts,
                                                                            double* __restrict__ stats) {
  double c = 0.0, m = 0.0, s = 0.0;
  for (int i = threadIdx.x; i < nparts; i += SURF_BLOCK) {
    c += partials[3 * i];
    m = fmax(m, partials[3 * i + 1]);
    s += partials[3 * i + 2];
  }
  __shared__ double red[SURF_BLOCK / 64][3];
  surf_stats_block_reduce(c, m, s, red);
  if (threadIdx.x == 0) {
    stats[0] = c;
    stats[1] = sqrt(m);
    stats[2] = s;
  }
}

// ---- workspace plan (pure host arithmetic of the volume size) --------------------------------------------------------
static inline int surf_grid(i64 items) {
  i64 g = (items + SURF_BLOCK - 1) / SURF_BLOCK;
  return (int)(g < 1 ? 1 : (g > SURF_MAX_BLOCKS ? SURF_MAX_BLOCKS : g));
}
static inline int surf_row_grid(int Y, int Z) {
  const i64 g = ((i64)Y * Z + SURF_BLOCK / 64 - 1) / (SURF_BLOCK / 64);
  return (int)(g > 8192 ? 8192 : g);
}

struct SurfWorkspace {
  i64 g, f2, st_s, st_t, st_f, partials, counter, total;   // byte offsets
};
static SurfWorkspace surf_plan(int X, int Y, int Z) {
  const i64 n = (i64)X * Y * Z;
  SurfWorkspace w;
  w.g = 0;
  w.f2 = w.g + surf_align(4 * n);
  w.st_s = w.f2 + surf_align(8 * n);
  w.st_t = w.st_s + surf_align(4 * n);
  w.st_f = w.st_t + surf_align(4 * n);
  w.partials = w.st_f + surf_align(8 * n);
  w.counter = w.partials + surf_align(3 * 8 * (i64)surf_grid((i64)X * Y));
  w.total = w.counter + 256;
  return w;
}

extern "C" long long seg3d_surface_distance_workspace_bytes(int X, int Y, int Z) {
  if (X <= 0 || Y <= 0 || Z <= 0 || (i64)X * Y * Z >= (1ll << 31)) return -1;
  return surf_plan(X, Y, Z).total;
}

extern "C" int seg3d_surface_distance(const unsigned char* feature_surface, const unsigned char* query_surface, int X,
                                      int Y, int Z, const int* box_device, double sx, double sy, double sz,
                                      void* workspace, double* dist2_out, int* index_out, long long capacity,
                                      double* stats, void* stream) {
  SEG3D_REQUIRE(feature_surface && query_surface && box_device && workspace && stats,
                "seg3d_surface_distance: null pointer");
  SEG3D_REQUIRE(X > 0 && Y > 0 && Z > 0 && (i64)X * Y * Z < (1ll << 31),
                "seg3d_surface_distance: bad volume size %d x %d x %d (1 .. 2^31 - 1 voxels)", X, Y, Z);
  SEG3D_REQUIRE(sx > 0.0 && sy > 0.0 && sz > 0.0 && sx < 1e30 && sy < 1e30 && sz < 1e30,
                "seg3d_surface_distance: spacing must be positive and finite (got %g, %g, %g)", sx, sy, sz);
  SEG3D_REQUIRE(capacity >= 0 && (capacity == 0 || dist2_out), "seg3d_surface_distance: bad output buffer");
  hipStream_t s = (hipStream_t)stream;
  const SurfWorkspace w = surf_plan(X, Y, Z);
  char* ws = (char*)workspace;
  int* g = (int*)(ws + w.g);
  double* f2 = (double*)(ws + w.f2);
  int* st_s = (int*)(ws + w.st_s);
  int* st_t = (int*)(ws + w.st_t);
  double* st_f = (double*)(ws + w.st_f);
  double* partials = (double*)(ws + w.partials);
  int* counter = (int*)(ws + w.counter);
  if (hipMemsetAsync(counter, 0, sizeof(int), s) != hipSuccess) {
    seg3d_set_error("seg3d_surface_distance: hipMemsetAsync failed");
    return SEG3D_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(edt_rows_kernel, dim3(surf_row_grid(Y, Z)), dim3(SURF_BLOCK), 0, s, feature_surface, box_device, X,
                     Y, Z, g);
  hipLaunchKernelGGL(edt_cols_y_kernel, dim3(surf_grid((i64)Z * X)), dim3(SURF_BLOCK), 0, s, (const int*)g, box_device,
                     X, Y, Z, sx * sx, sy * sy, st_s, st_t, st_f, f2);
  const int nparts = surf_grid((i64)X * Y);
  hipLaunchKernelGGL(edt_cols_z_query_kernel, dim3(nparts), dim3(SURF_BLOCK), 0, s, (const double*)f2, query_surface,
                     box_device, X, Y, Z, sz * sz, st_s, st_t, st_f, counter, dist2_out, index_out, (i64)capacity, partials);
  hipLaunchKernelGGL(surface_stats_finalize_kernel, dim3(1), dim3(SURF_BLOCK), 0, s, (const double*)partials, nparts,
                     stats);
  SEG3D_LAUNCH_CHECK("seg3d_surface_distance");
  return SEG3D_OK;
}
