// lesion.hip -- device side of the lesion-wise evaluation (lesion-wise Dice / HD95 as BraTS has ranked since 2023; no
// counterpart in the reference; definitions in DESIGN.md section 7 row f18 and include/seg3d_hip.h).
//
// For a target (a set of label ids in 1..255): A = ground-truth voxels in the set, B = segmentation voxels in the set.
//   seg3d_label_set_mask    label volume (five dtypes) + 256-bit set  ->  0/1 byte mask
//   seg3d_binary_dilate18   A' = A dilated by the 18-neighbourhood, one launch per iteration
//   (seg3d_ccl26_label, postproc.hip: Dmap = canonical components of A', Pmap = those of B)
//   seg3d_lesion_pairs      one pass over (Dmap, A, Pmap): |G_i|, |G_i n B| and the set of distinct (i, j) with Dmap = i,
//                           Pmap = j, in an open-addressing hash set
//   seg3d_lesion_select     the two masks of lesion i, g = (Dmap == i) & A and u = flag[Pmap], for the surface entries
// Everything is integer work with integer atomics: exact and identical from run to run.  No workgroup waits on another;
// every loop has a bound known at launch.  All five are HBM byte movers.
#include "label_device.h"
#include "seg3d_hip.h"

// ---- set membership ---------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ bool lesion_in_set(T x, const Seg3dLabelSet& set) {
  const int l = label_byte<T>(x);
  return l >= 0 && ((set.bits[l >> 5] >> (l & 31)) & 1u);
}

template <typename T>
__global__ __launch_bounds__(256) void label_set_mask_kernel(const T* __restrict__ vol, i64 n, Seg3dLabelSet set,
                                                              unsigned char* __restrict__ mask) {
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256)
    mask[i] = lesion_in_set<T>(vol[i], set) ? 1 : 0;
}

extern "C" int seg3d_label_set_mask(const void* labels, int dtype, long long n, Seg3dLabelSet set, unsigned char* mask,
                                    void* stream) {
  SEG3D_REQUIRE(labels && mask, "seg3d_label_set_mask: null pointer");
  SEG3D_REQUIRE(n > 0 && n < (1ll << 31), "seg3d_label_set_mask: bad element count %lld (1 .. 2^31 - 1)", n);
  const int rc = label_dispatch(dtype, "seg3d_label_set_mask", [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((label_set_mask_kernel<T>), dim3(seg3d_ew_grid(n, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const T*)labels, (i64)n, set, mask);
  });
  if (rc != SEG3D_OK) return rc;
  SEG3D_LAUNCH_CHECK("seg3d_label_set_mask");
  return SEG3D_OK;
}

// ---- one dilation by the 18-neighbourhood --------------------------------------------------------------------------------
// The tile is cldice_loss.hip's 32 x 8 x 8: of the 2048-voxel tiles with a row of at least 32 voxels it stages the
// fewest halo voxels (34 x 10 x 10 = 3400, 1.66 loads per voxel), a workgroup's 256 threads map to one 32 x 8 plane, and
// thread (lx, ly) walks its column of 8 voxels along z, so the in-plane ORs of a staged plane are taken once and serve
// the three outputs that read the plane.  Staged bytes are 0 outside the volume: nothing exists there.
// A voxel of plane z sees the full 3 x 3 of its own plane (P9) and the centre + 4 face neighbours (P5) of planes z -+ 1:
// exactly the offsets with at most two non-zero components.
#define LES_TX 32
#define LES_TY 8
#define LES_TZ 8
#define LES_HX (LES_TX + 2)
#define LES_HY (LES_TY + 2)
#define LES_HZ (LES_TZ + 2)
#define LES_PITCH 36   // staged row pitch in bytes (a multiple of the 4-byte bank)

__global__ __launch_bounds__(256) void dilate18_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                        int X, int Y, int Z, int ntx, int nty) {
  __shared__ unsigned char tile[LES_HZ * LES_HY * LES_PITCH];
  const int b = blockIdx.x;
  const int x0 = (b % ntx) * LES_TX, y0 = ((b / ntx) % nty) * LES_TY, z0 = (b / (ntx * nty)) * LES_TZ;
  for (int i = threadIdx.x; i < LES_HX * LES_HY * LES_HZ; i += 256) {
    const int lx = i % LES_HX, ly = (i / LES_HX) % LES_HY, lz = i / (LES_HX * LES_HY);
    const int x = x0 - 1 + lx, y = y0 - 1 + ly, z = z0 - 1 + lz;
    const bool in = x >= 0 && x < X && y >= 0 && y < Y && z >= 0 && z < Z;
    tile[(lz * LES_HY + ly) * LES_PITCH + lx] = (in && src[((i64)z * Y + y) * X + x]) ? 1 : 0;
  }
  __syncthreads();
  const int lx = threadIdx.x & (LES_TX - 1), ly = threadIdx.x / LES_TX;
  const int x = x0 + lx, y = y0 + ly;
  if (x >= X || y >= Y) return;   // after the only barrier
  unsigned p5[LES_HZ], p9[LES_HZ];
#pragma unroll
  for (int lz = 0; lz < LES_HZ; ++lz) {
    const unsigned char* r0 = tile + (lz * LES_HY + ly) * LES_PITCH + lx;   // row y - 1, column x - 1
    const unsigned char* r1 = r0 + LES_PITCH;
    const unsigned char* r2 = r1 + LES_PITCH;
    p5[lz] = r1[0] | r1[1] | r1[2] | r0[1] | r2[1];
    p9[lz] = p5[lz] | r0[0] | r0[2] | r2[0] | r2[2];
  }
#pragma unroll
  for (int k = 0; k < LES_TZ; ++k) {
    const int z = z0 + k;
    if (z < Z) dst[((i64)z * Y + y) * X + x] = (p5[k] | p9[k + 1] | p5[k + 2]) ? 1 : 0;
  }
}

extern "C" int seg3d_binary_dilate18(const unsigned char* mask, unsigned char* out, unsigned char* workspace, int X, int Y,
                                     int Z, int iters, void* stream) {
  SEG3D_REQUIRE(mask && out, "seg3d_binary_dilate18: null pointer");
  SEG3D_REQUIRE(X > 0 && Y > 0 && Z > 0 && (i64)X * Y * Z < (1ll << 31),
                "seg3d_binary_dilate18: bad volume size %d x %d x %d (1 .. 2^31 - 1 voxels)", X, Y, Z);
  SEG3D_REQUIRE(iters >= 0 && iters <= 16, "seg3d_binary_dilate18: %d iterations, 0..16 are supported", iters);
  SEG3D_REQUIRE(iters < 2 || workspace, "seg3d_binary_dilate18: %d iterations need the workspace plane", iters);
  SEG3D_REQUIRE(mask != out && (iters < 2 || (workspace != out && workspace != mask)),
                "seg3d_binary_dilate18: input, output and workspace must be distinct buffers");
  hipStream_t s = (hipStream_t)stream;
  const i64 total = (i64)X * Y * Z;
  if (iters == 0) {
    if (hipMemcpyAsync(out, mask, (size_t)total, hipMemcpyDeviceToDevice, s) != hipSuccess) {
      seg3d_set_error("seg3d_binary_dilate18: hipMemcpyAsync failed");
      return SEG3D_ERR_LAUNCH;
    }
    return SEG3D_OK;
  }
  const int ntx = seg3d_cdiv(X, LES_TX), nty = seg3d_cdiv(Y, LES_TY), ntz = seg3d_cdiv(Z, LES_TZ);
  const i64 tiles = (i64)ntx * nty * ntz;   // <= 2^31 / 2048 * (padding of partial tiles) -- checked below
  SEG3D_REQUIRE(tiles < (1ll << 31), "seg3d_binary_dilate18: %lld tiles exceed the grid limit", tiles);
  const unsigned char* src = mask;
  for (int k = 0; k < iters; ++k) {   // the last iteration (iters - 1 - k == 0) lands in out
    unsigned char* dst = ((iters - 1 - k) & 1) ? workspace : out;
    hipLaunchKernelGGL(dilate18_kernel, dim3((unsigned)tiles), dim3(256), 0, s, src, dst, X, Y, Z, ntx, nty);
    src = dst;
  }
  SEG3D_LAUNCH_CHECK("seg3d_binary_dilate18");
  return SEG3D_OK;
}

// ---- per-lesion counts and the (lesion, predicted component) pair set -----------------------------------------------------
// A wave takes 64 consecutive voxels per step.  Lanes with equal (i, j) are collapsed before anything global happens: the
// first lane of each distinct key adds the popcounts to gsize[i] / inter[i] and inserts the key once, so a wave inside one
// lesion issues two or three atomics per step instead of up to 192 on the same two addresses.  At most 64 rounds per step.
// Measured on the 240 x 240 x 155 case of tools/bench_lesionwise.py against one set of atomics per voxel: see DESIGN.md.
// Hash set: 64-bit keys (i << 32 | j, never 0), 0 = empty, atomicCAS insert, linear probing with at most `capacity`
// probes.  A key that finds no slot sets the status word; inserts that start after that are skipped (the host doubles the
// table and repeats the launch anyway), the counts are complete either way.
__device__ __forceinline__ unsigned long long lesion_hash(unsigned long long k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

// one key into the set; the status word is set when every slot holds another key
__device__ __forceinline__ void lesion_insert(unsigned long long* __restrict__ table, unsigned long long cap_mask,
                                              unsigned long long key, int* __restrict__ status) {
  bool done = *(volatile int*)status != 0;   // table already known to be too small: the launch is repeated
  unsigned long long slot = lesion_hash(key) & cap_mask;
  for (unsigned long long probe = 0; !done && probe <= cap_mask; ++probe) {
    const unsigned long long old = atomicCAS(table + slot, 0ull, key);
    done = old == 0ull || old == key;
    slot = (slot + 1) & cap_mask;
  }
  if (!done) atomicOr(status, 1);
}

// COLLAPSE = false: every voxel issues its own atomics and its own insert (kept for the measurement in
// tools/bench_lesionwise.py; the results are the same integers)
template <bool COLLAPSE>
__global__ __launch_bounds__(256) void lesion_pairs_kernel(const int* __restrict__ dmap, const unsigned char* __restrict__ a,
                                                            const int* __restrict__ pmap, i64 n, int kg,
                                                            unsigned long long* __restrict__ gsize,
                                                            unsigned long long* __restrict__ inter,
                                                            unsigned long long* __restrict__ table, unsigned long long cap_mask,
                                                            int* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  for (i64 base = (i64)blockIdx.x * 256; base < n; base += (i64)gridDim.x * 256) {   // uniform over the workgroup
    const i64 idx = base + threadIdx.x;
    int i = 0, j = 0;
    bool ina = false;
    if (idx < n) {
      i = dmap[idx];
      if (i > 0 && i <= kg) {
        const int p = pmap[idx];
        j = p > 0 ? p : 0;
        ina = a[idx] != 0;
      } else {
        i = 0;
      }
    }
    const unsigned long long key = ((unsigned long long)(unsigned)i << 32) | (unsigned)j;
    if constexpr (!COLLAPSE) {
      if (i > 0) {
        if (ina) atomicAdd(gsize + i, 1ull);
        if (j > 0) {
          if (ina) atomicAdd(inter + i, 1ull);
          lesion_insert(table, cap_mask, key, status);
        }
      }
    } else {
      const unsigned long long in_a = __ballot(ina);
      unsigned long long todo = __ballot(i > 0);
      while (todo) {   // one round per distinct key of the wave: todo loses at least its lowest bit every round
        const int leader = __ffsll(todo) - 1;
        const unsigned long long k = __shfl(key, leader, 64);
        const unsigned long long same = __ballot(i > 0 && key == k);
        if (lane == leader) {
          const unsigned long long cnt = (unsigned long long)__popcll(same & in_a);
          if (cnt) atomicAdd(gsize + i, cnt);
          if (j > 0) {
            if (cnt) atomicAdd(inter + i, cnt);
            lesion_insert(table, cap_mask, key, status);
          }
        }
        todo &= ~same;
      }
    }
  }
}

extern "C" int seg3d_lesion_pairs(const int* dmap, const unsigned char* a, const int* pmap, long long n, int kg,
                                  long long* gsize, long long* inter, unsigned long long* table, long long capacity,
                                  int collapse, int* status, void* stream) {
  SEG3D_REQUIRE(dmap && a && pmap && gsize && inter && table && status, "seg3d_lesion_pairs: null pointer");
  SEG3D_REQUIRE(n > 0 && n < (1ll << 31), "seg3d_lesion_pairs: bad element count %lld (1 .. 2^31 - 1)", n);
  SEG3D_REQUIRE(kg >= 0, "seg3d_lesion_pairs: negative lesion count %d", kg);
  SEG3D_REQUIRE(capacity >= 1 && capacity <= (1ll << 40) && (capacity & (capacity - 1)) == 0,
                "seg3d_lesion_pairs: table capacity %lld is not a power of two", capacity);
  i64 blocks = (n + 256 * 8 - 1) / (256 * 8);
  if (blocks > 8192) blocks = 8192;
  const dim3 grid((unsigned)blocks);
  unsigned long long* gs = (unsigned long long*)gsize;
  unsigned long long* in = (unsigned long long*)inter;
  const unsigned long long cap_mask = (unsigned long long)(capacity - 1);
  if (collapse)
    hipLaunchKernelGGL(lesion_pairs_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, dmap, a, pmap, (i64)n, kg, gs, in,
                       table, cap_mask, status);
  else
    hipLaunchKernelGGL(lesion_pairs_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, dmap, a, pmap, (i64)n, kg, gs, in,
                       table, cap_mask, status);
  SEG3D_LAUNCH_CHECK("seg3d_lesion_pairs");
  return SEG3D_OK;
}

// ---- the two masks of one lesion ------------------------------------------------------------------------------------------
// Whole volume: a box per lesion would need per-component boxes from another pass, and the passes that follow
// (seg3d_label_surface, seg3d_surface_distance) confine themselves to the box of the two surfaces already.
__global__ __launch_bounds__(256) void lesion_select_kernel(const int* __restrict__ dmap, const unsigned char* __restrict__ a,
                                                             const int* __restrict__ pmap,
                                                             const unsigned char* __restrict__ flag, int kp, int lesion, i64 n,
                                                             unsigned char* __restrict__ g, unsigned char* __restrict__ u) {
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
    g[i] = (dmap[i] == lesion && a[i]) ? 1 : 0;
    const int p = pmap[i];
    u[i] = (p > 0 && p <= kp && flag[p]) ? 1 : 0;
  }
}

extern "C" int seg3d_lesion_select(const int* dmap, const unsigned char* a, const int* pmap, const unsigned char* flag,
                                   int kp, int lesion, long long n, unsigned char* g, unsigned char* u, void* stream) {
  SEG3D_REQUIRE(dmap && a && pmap && flag && g && u, "seg3d_lesion_select: null pointer");
  SEG3D_REQUIRE(n > 0 && n < (1ll << 31), "seg3d_lesion_select: bad element count %lld (1 .. 2^31 - 1)", n);
  SEG3D_REQUIRE(kp >= 0 && lesion >= 1, "seg3d_lesion_select: bad component count %d or lesion id %d", kp, lesion);
  hipLaunchKernelGGL(lesion_select_kernel, dim3(seg3d_ew_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, dmap, a, pmap,
                     flag, kp, lesion, (i64)n, g, u);
  SEG3D_LAUNCH_CHECK("seg3d_lesion_select");
  return SEG3D_OK;
}
