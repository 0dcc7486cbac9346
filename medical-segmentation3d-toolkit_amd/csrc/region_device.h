// region_device.h -- what the kernels of region-based training share: the region loss (region_loss.hip) and the region
// confusion counts of the validation pass (validation.hip).  Definitions: DESIGN.md section 7, row f23.
//   table          256 words, bit r of word l set iff label l belongs to region r (loss/region_loss.py region_lut); it travels
//                  BY VALUE in the kernel arguments (1 KB; a captured graph bakes it in) and is staged in LDS, as
//                  overlap_kernel of metrics.hip does
//   counting rule  l = label_byte(t) (label_device.h: the integer in [0, 256), else -1); a voxel counts iff l >= 0 &&
//                  t != ignore, so any ignore outside [0, 256) means none; the target of region r is (table[l] >> r) & 1
#pragma once
#include "label_device.h"

struct RegionLut {
  unsigned v[256];
#ifdef __HIPCC__
  // every thread of a workgroup of >= 256 threads calls this once, first thing
  __device__ __forceinline__ const unsigned* stage() const {
    __shared__ unsigned lut[256];
    if (threadIdx.x < 256) lut[threadIdx.x] = v[threadIdx.x];
    __syncthreads();
    return lut;
  }
#endif
};

static inline RegionLut region_table(const unsigned* lut_host) {
  RegionLut m;
  for (int k = 0; k < 256; ++k) m.v[k] = lut_host[k];
  return m;
}

#ifdef __HIPCC__
// the membership word of a target value (at most 16 bits), -1 if the voxel does not count
__device__ __forceinline__ int region_bits(const unsigned* lut, float t, float ignore) {
  const int l = label_byte<float>(t);
  return (l >= 0 && t != ignore) ? (int)lut[l] : -1;
}
#endif
