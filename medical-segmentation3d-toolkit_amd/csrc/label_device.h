// label_device.h -- what the evaluation kernels share: metrics.hip (overlap counts), surface.hip (surface extraction),
// lesion.hip (set masks) and postproc.hip (bounding box).  They read label volumes as the file formats store them:
//   dtype code   0 = int8, 1 = uint8, 2 = int16, 3 = int32, 4 = float32      (label_dispatch: code -> element type)
//   set rule     a value that is no integer in [0, 256) belongs to no set    (label_byte)
//   box          min / max of (x, y, z) over selected voxels, wave-reduced, one set of atomics per wave  (LabelBox)
#pragma once
#include <limits.h>

#include "seg3d_common.h"

// launch(T()) for the element type T behind `dtype`; `launch` is a generic lambda that reads only the type of its argument.
// An unknown code sets "<entry>: unknown dtype code <dtype>" and returns SEG3D_ERR_UNSUPPORTED.
template <typename F>
static inline int label_dispatch(int dtype, const char* entry, F&& launch) {
  switch (dtype) {
    case 0: launch((signed char)0); return SEG3D_OK;
    case 1: launch((unsigned char)0); return SEG3D_OK;
    case 2: launch((short)0); return SEG3D_OK;
    case 3: launch((int)0); return SEG3D_OK;
    case 4: launch(0.0f); return SEG3D_OK;
    default: SEG3D_UNSUPPORTED("%s: unknown dtype code %d", entry, dtype);
  }
}

#ifdef __HIPCC__
// the label as an int in [0, 256), or -1 when x is not such an integer
template <typename T>
__device__ __forceinline__ int label_byte(T x) {
  const float f = (float)x;   // exact for every value in [0, 256) of the five types; larger ints may round but stay >= 256
  return (f >= 0.0f && f < 256.0f && f == floorf(f)) ? (int)f : -1;
}

// box[6] = (xmin, ymin, zmin, xmax, ymax, zmax), inclusive; the caller initialises it to {INT_MAX x 3, -1 x 3}
struct LabelBox {
  int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {-1, -1, -1};
  __device__ __forceinline__ void add(int x, int y, int z) {
    lo[0] = min(lo[0], x); lo[1] = min(lo[1], y); lo[2] = min(lo[2], z);
    hi[0] = max(hi[0], x); hi[1] = max(hi[1], y); hi[2] = max(hi[2], z);
  }
  // every thread of the workgroup calls this once, after its walk; a wave that added nothing leaves the box untouched
  __device__ __forceinline__ void wave_commit(int* __restrict__ box) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        lo[d] = min(lo[d], __shfl_down(lo[d], off, 64));
        hi[d] = max(hi[d], __shfl_down(hi[d], off, 64));
      }
    }
    if ((threadIdx.x & 63) == 0 && hi[0] >= 0) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        atomicMin(box + d, lo[d]);
        atomicMax(box + 3 + d, hi[d]);
      }
    }
  }
};
#endif
