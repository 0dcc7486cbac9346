// mc_device.h -- what the multi-modality ("mc") kernels share: patch.hip (gather), postproc.hip (resampler), augment.hip
// (intensity) and augment_filter.hip (blur, low-resolution simulation).  They work on channels-last voxel rows
// [z][y][x][M], M <= 8 co-registered modalities, and are instantiated per row width:
//   MC = 1, 2, 3, 4  compile-time width; VEC (MC = 4 / 2 only): a row is one 16- / 8-byte access
//   MC = 0           runtime width M <= 8, rows of MR = 8 registers, scalar accesses guarded by m < M
// Every kernel does the same arithmetic per (voxel, modality) whatever the instantiation, so channel m of an M-channel call
// equals the M = 1 call on plane m bit for bit.
//   width            mc_regs<MC> (MR), mc_width<MC>(M)
//   rows             mc_load_row / mc_store_row: the load fills the registers past M with a value of the caller's, the
//                    store writes m < M only
//   typed rows       mc_load_row / mc_load_elem of a short / unsigned char / signed char source (the resampler's compact
//                    volumes): the same registers, every element through (float)
//   host             mc_vec_rows (may the rows be moved as vectors?; mc_vec_rows_typed for a typed source) and MC_DISPATCH
//                    ((M, vec) -> <MC, VEC>)
//   statistics       mc_chunk_walk (MC_STAT_CHUNK voxels per workgroup, 256 threads) and the fixed-order fp64 block sum
//                    mc_stat_park -> barrier -> mc_stat_total of patch_stats_partial_mc_kernel and augment_stats_partial_kernel
// Left local on purpose: the trilinear branch of resample_affine_mc_kernel at MC = 0 reads its eight rows channel by channel
// (p000[m] ... p111[m]) -- eight rows of eight floats through mc_load_row would hold 64 registers; and
// augment_blur_kernel splits M otherwise (4 / 2 channels per workgroup on vector rows, else one channel per workgroup with
// grid y = M), so it takes mc_vec_rows but not MC_DISPATCH.
#pragma once
#include "seg3d_common.h"

#define MC_STAT_CHUNK 8192  // voxels per workgroup of the chunked statistics passes

// rows of M floats can be moved as one access: M == 4 and every base 16-byte aligned, or M == 2 and 8-byte aligned; a voxel
// stride other than M must be a multiple of M
static inline bool mc_vec_rows(int M, const void* a, const void* b = nullptr, i64 stride = 0) {
  if (M != 4 && M != 2) return false;
  return (((uintptr_t)a | (uintptr_t)b) & (uintptr_t)(4 * M - 1)) == 0 && stride % M == 0;
}

// mc_vec_rows for a launch that reads rows of M elements of `src_elem` bytes and writes rows of M floats: the source base
// must be aligned to its row's bytes (2-byte elements: one 8-byte access at M = 4, one 4-byte access at M = 2), the
// destination rule is the one above; 1-byte elements take scalar loads.  src_elem = 4 is mc_vec_rows(M, src, dst, stride).
static inline bool mc_vec_rows_typed(int M, const void* src, size_t src_elem, const void* dst, i64 stride) {
  if (src_elem < 2) return false;
  return mc_vec_rows(M, nullptr, dst, stride) && ((uintptr_t)src & (uintptr_t)(src_elem * M - 1)) == 0;
}

// F<MC, VEC> __VA_ARGS__ for the instantiation of (M, vec); F may carry a leading `return`
#define MC_DISPATCH(F, M, vec, ...)                                                          \
  do {                                                                                       \
    switch (M) {                                                                             \
      case 1: F<1, false> __VA_ARGS__; break;                                                \
      case 4: if (vec) F<4, true> __VA_ARGS__; else F<4, false> __VA_ARGS__; break;          \
      case 2: if (vec) F<2, true> __VA_ARGS__; else F<2, false> __VA_ARGS__; break;          \
      case 3: F<3, false> __VA_ARGS__; break;                                                \
      default: F<0, false> __VA_ARGS__; break;                                               \
    }                                                                                        \
  } while (0)

#ifdef __HIPCC__
template <int MC>
constexpr int mc_regs = MC > 0 ? MC : 8;  // registers of a row
template <int MC>
__device__ __forceinline__ int mc_width(int Mrt) { return MC > 0 ? MC : Mrt; }

// a row of compile-time width.  VEC: one 16- / 8-byte access (the launcher guarantees the alignment, mc_vec_rows)
template <int MC, bool VEC>
__device__ __forceinline__ void mc_load_row(const float* p, float* v) {
  static_assert(MC > 0, "the runtime width needs M and a fill value");
  if constexpr (VEC && MC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else if constexpr (VEC && MC == 2) {
    const float2 t = *reinterpret_cast<const float2*>(p);
    v[0] = t.x; v[1] = t.y;
  } else {
#pragma unroll
    for (int m = 0; m < MC; ++m) v[m] = p[m];
  }
}
template <int MC, bool VEC>
__device__ __forceinline__ void mc_store_row(float* p, const float* v) {
  static_assert(MC > 0, "the runtime width needs M");
  if constexpr (VEC && MC == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else if constexpr (VEC && MC == 2) {
    *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
  } else {
#pragma unroll
    for (int m = 0; m < MC; ++m) p[m] = v[m];
  }
}

// a row of any width, M = mc_width<MC>(...): v[0 .. mc_regs<MC>) = the row, `fill` past M; the store writes m < M
template <int MC, bool VEC>
__device__ __forceinline__ void mc_load_row(const float* p, float* v, int M, float fill) {
  if constexpr (MC > 0) {
    mc_load_row<MC, VEC>(p, v);
  } else {
#pragma unroll
    for (int m = 0; m < 8; ++m) v[m] = m < M ? p[m] : fill;
  }
}
template <int MC, bool VEC>
__device__ __forceinline__ void mc_store_row(float* p, const float* v, int M) {
  if constexpr (MC > 0) {
    mc_store_row<MC, VEC>(p, v);
  } else {
#pragma unroll
    for (int m = 0; m < 8; ++m)
      if (m < M) p[m] = v[m];
  }
}

// ---- typed source rows (the resampler reads volumes as the files store them): SRC = short, unsigned char or signed
// char; every element goes through (float), which is exact for these types, into the registers the float overloads fill.
// VEC is honoured for 2-byte elements only (the launcher never asks for it otherwise, mc_vec_rows_typed).
template <int MC, bool VEC, typename SRC>
__device__ __forceinline__ void mc_load_row(const SRC* p, float* v) {
  static_assert(MC > 0, "the runtime width needs M and a fill value");
  static_assert(sizeof(SRC) <= 2, "float rows take the overload above");
  if constexpr (VEC && MC == 4 && sizeof(SRC) == 2) {
    const short4 t = *reinterpret_cast<const short4*>(p);
    v[0] = (float)t.x; v[1] = (float)t.y; v[2] = (float)t.z; v[3] = (float)t.w;
  } else if constexpr (VEC && MC == 2 && sizeof(SRC) == 2) {
    const short2 t = *reinterpret_cast<const short2*>(p);
    v[0] = (float)t.x; v[1] = (float)t.y;
  } else {
#pragma unroll
    for (int m = 0; m < MC; ++m) v[m] = (float)p[m];
  }
}
template <int MC, bool VEC, typename SRC>
__device__ __forceinline__ void mc_load_row(const SRC* p, float* v, int M, float fill) {
  if constexpr (MC > 0) {
    mc_load_row<MC, VEC>(p, v);
  } else {
#pragma unroll
    for (int m = 0; m < 8; ++m) v[m] = m < M ? (float)p[m] : fill;
  }
}
// channel m of a row as a float: the runtime width's trilinear branch reads its eight rows channel by channel
template <typename SRC>
__device__ __forceinline__ float mc_load_elem(const SRC* p, int m) { return (float)p[m]; }

// ---- chunked statistics: workgroup blockIdx.x of 256 threads owns voxels [blockIdx.x * MC_STAT_CHUNK, + MC_STAT_CHUNK) of
// nv; thread i takes e = e0 + i, e0 + 256 + i, ...: row_of(e) is the voxel's row, acc(r) adds its registers (0 past M) to the
// thread's accumulators
template <int MC, bool VEC, typename RowOf, typename Acc>
__device__ __forceinline__ void mc_chunk_walk(i64 nv, int M, RowOf row_of, Acc acc) {
  const i64 e0 = (i64)blockIdx.x * MC_STAT_CHUNK;
  i64 e1 = e0 + MC_STAT_CHUNK;
  if (e1 > nv) e1 = nv;
  for (i64 e = e0 + threadIdx.x; e < e1; e += 256) {
    float r[mc_regs<MC>];
    mc_load_row<MC, VEC>(row_of(e), r, M, 0.f);
    acc(r);
  }
}

// the block sum of per-modality fp64 accumulators in a fixed order: wave reduce, lane 0 of wave w parks the wave's value in
// slot[m][first + w]; after a __syncthreads() thread m adds the four slots left to right
template <int MR, int NS>
__device__ __forceinline__ void mc_stat_park(double (&v)[MR], double (&slot)[MR][NS], int first) {
#pragma unroll
  for (int m = 0; m < MR; ++m) v[m] = wave_sum_d(v[m]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int m = 0; m < MR; ++m) slot[m][first + (threadIdx.x >> 6)] = v[m];
  }
}
__device__ __forceinline__ double mc_stat_total(const double* slot) { return slot[0] + slot[1] + slot[2] + slot[3]; }
#endif
