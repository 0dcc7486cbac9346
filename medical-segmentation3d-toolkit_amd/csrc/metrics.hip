// metrics.hip -- label-overlap counts for the Dice evaluation metric.
//
// Reference restated (file:line relative to /root/reference/segmentation3d):  utils/metrics.py:5-37 `cal_dsc`
//   gt == label, seg == label, area_gt = sum, area_seg = sum, intersection = sum(gt & seg)
// evaluated by core/seg_eval.py:8-57 once per (case, label), i.e. three full passes over both volumes per label on
// the host.  Here ONE pass over the two label volumes yields (area_gt, area_seg, intersection) for all requested
// labels: integer counting, bit-exact, HBM-bound (algorithmic bytes = 2 * voxels * element size).
// The region counts are the same pass with set membership in place of equality: one
// kernel, overlap_kernel<T, Member>; a Member supplies what it stages per workgroup, the key of a voxel and how the keys
// of a voxel pair are tallied for set k.
#include "label_device.h"
#include "seg3d_hip.h"

#define METRIC_MAX_SETS 16   // labels or regions per pass

// set k = { x : x == labels[k] }, compared in the volume's own type: a voxel's key is its value
struct LabelMember {
  int v[METRIC_MAX_SETS];
  __device__ __forceinline__ const int* stage() const { return v; }
  template <typename T>
  static __device__ __forceinline__ T key(const int*, T x) { return x; }
  // g and s by reference on purpose: by-value parameters are known to be defined, which turns a && b into a bitwise and
  // and all three updates of the int8 / int16 kernels into carry adds writing SGPR pairs; measured on the MI355X that
  // form is 7 % slower with 16 labels on int8 volumes (profiles/eval_rows_ab.json)
  template <typename T>
  static __device__ __forceinline__ void tally(const int* labels, int k, const T& g, const T& s, unsigned& cg, unsigned& cs,
                                               unsigned& ci) {
    const T l = (T)labels[k];
    const bool a = g == l, b = s == l;
    cg += a ? 1u : 0u;
    cs += b ? 1u : 0u;
    ci += (a && b) ? 1u : 0u;
  }
};

// set k = region k: bit r of v[l] = label l belongs to region r (label_byte's rule for what a label is).  The LUT is staged
// in LDS; a voxel's key is its LUT word.
struct RegionMember {
  unsigned v[256];
  __device__ __forceinline__ const unsigned* stage() const {
    __shared__ unsigned lut[256];
    lut[threadIdx.x] = v[threadIdx.x];
    __syncthreads();
    return lut;
  }
  template <typename T>
  static __device__ __forceinline__ unsigned key(const unsigned* lut, T x) {
    const int l = label_byte<T>(x);
    return l >= 0 ? lut[l] : 0u;
  }
  static __device__ __forceinline__ void tally(const unsigned*, int k, unsigned g, unsigned s, unsigned& cg, unsigned& cs,
                                               unsigned& ci) {
    const unsigned b = g & s;
    cg += (g >> k) & 1u;
    cs += (s >> k) & 1u;
    ci += (b >> k) & 1u;
  }
};

template <typename T, typename Member>
__global__ __launch_bounds__(256) void overlap_kernel(const T* __restrict__ gt, const T* __restrict__ seg, i64 n, Member member,
                                                       int nsets, unsigned long long* __restrict__ counts) {
  const auto staged = member.stage();
  unsigned cg[METRIC_MAX_SETS], cs[METRIC_MAX_SETS], ci[METRIC_MAX_SETS];
#pragma unroll
  for (int k = 0; k < METRIC_MAX_SETS; ++k) cg[k] = cs[k] = ci[k] = 0u;
  // a thread visits at most 2^31 / (gridDim * 256) elements: 32-bit per-thread counters cannot overflow for n < 2^40
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
    const auto g = Member::key(staged, gt[i]), s = Member::key(staged, seg[i]);
#pragma unroll
    for (int k = 0; k < METRIC_MAX_SETS; ++k)
      if (k < nsets) Member::tally(staged, k, g, s, cg[k], cs[k], ci[k]);
  }
  __shared__ unsigned red[4][METRIC_MAX_SETS * 3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < METRIC_MAX_SETS; ++k) {
    if (k < nsets) {
      unsigned a = cg[k], b = cs[k], c = ci[k];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_down(a, off, 64);
        b += __shfl_down(b, off, 64);
        c += __shfl_down(c, off, 64);
      }
      if (lane == 0) {
        red[wave][3 * k] = a;
        red[wave][3 * k + 1] = b;
        red[wave][3 * k + 2] = c;
      }
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < 3 * nsets) {
    const unsigned long long v = (unsigned long long)red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] +
                                 red[3][threadIdx.x];
    if (v) atomicAdd(counts + threadIdx.x, v);   // integer atomics: the result does not depend on the order
  }
}

// the two entries' common checks; `sets` is the entry's word for them ("labels" / "regions")
static int overlap_check(const char* name, const char* sets, const void* gt, const void* seg, const void* table_host,
                         const void* counts, long long n, int nsets) {
  SEG3D_REQUIRE(gt && seg && table_host && counts, "%s: null pointer", name);
  SEG3D_REQUIRE(n > 0 && n < (1ll << 40), "%s: bad element count", name);
  SEG3D_REQUIRE(nsets > 0 && nsets <= METRIC_MAX_SETS, "%s: 1..%d %s per call (got %d)", name, METRIC_MAX_SETS, sets, nsets);
  return SEG3D_OK;
}

template <typename Member>
static int overlap_launch(const char* name, const void* gt, const void* seg, int dtype, i64 n, const Member& member, int nsets,
                          unsigned long long* counts, void* stream) {
  i64 blocks = (n + 256 * 16 - 1) / (256 * 16);   // >= 16 elements per thread
  if (blocks > 256 * 16) blocks = 256 * 16;
  if (blocks < 1) blocks = 1;
  const int rc = label_dispatch(dtype, name, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((overlap_kernel<T, Member>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const T*)gt,
                       (const T*)seg, n, member, nsets, counts);
  });
  if (rc != SEG3D_OK) return rc;
  SEG3D_LAUNCH_CHECK(name);
  return SEG3D_OK;
}

// counts[k] = (area_gt, area_seg, intersection) of labels[k]; the caller zeroes `counts` (3 * nlabels u64) first.
// dtype: the codes of label_device.h (label volumes as the formats store them).
extern "C" int seg3d_label_overlap_counts(const void* gt, const void* seg, int dtype, long long n, const int* labels_host,
                                          int nlabels, unsigned long long* counts, void* stream) {
  const int rc = overlap_check("seg3d_label_overlap_counts", "labels", gt, seg, labels_host, counts, n, nlabels);
  if (rc != SEG3D_OK) return rc;
  LabelMember m;
  for (int k = 0; k < METRIC_MAX_SETS; ++k) m.v[k] = k < nlabels ? labels_host[k] : 0;
  return overlap_launch("seg3d_label_overlap_counts", gt, seg, dtype, n, m, nlabels, counts, stream);
}

// counts[3r..3r+2] += (|gt in region r|, |seg in region r|, |both|); the caller zeroes `counts` (3 * nregions u64) first.
// lut_host: 256 host words, bit r of lut_host[l] set iff label l is in region r; dtype codes as above.
extern "C" int seg3d_region_overlap_counts(const void* gt, const void* seg, int dtype, long long n, const unsigned* lut_host,
                                           int nregions, unsigned long long* counts, void* stream) {
  const int rc = overlap_check("seg3d_region_overlap_counts", "regions", gt, seg, lut_host, counts, n, nregions);
  if (rc != SEG3D_OK) return rc;
  RegionMember m;
  for (int k = 0; k < 256; ++k) m.v[k] = lut_host[k];
  return overlap_launch("seg3d_region_overlap_counts", gt, seg, dtype, n, m, nregions, counts, stream);
}
