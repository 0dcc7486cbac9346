// adam.hip -- fused optimizer steps over one flat fp32 parameter buffer: Adam with its scalars as launch arguments (the
// one-call entry), and the control-block family -- step count, gradient-norm clipping, learning-rate schedules on the
// device -- for Adam and SGD (second half of the file).
//
// Reference: optim.Adam(net.parameters(), lr, betas) + opt.step() (core/seg_train.py:83,127); defaults eps 1e-8,
// weight_decay 0, amsgrad off.  Update rule restated from torch.optim.Adam (single-tensor path):
//   g += wd * p;  m = lerp(m, g, 1-b1);  v = b2 v + (1-b2) g g;
//   p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// HBM-bound: 4 reads + 3 writes of 4 B per parameter (28 B/param; 0.41 GB for the 14.56 M-parameter V-Net).
#include "seg3d_common.h"
#include "seg3d_hip.h"

__device__ __forceinline__ void adam_step_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                               float* __restrict__ v, i64 n, float lr, float beta1, float beta2, float eps,
                                               float weight_decay, float bc1, float bc2_sqrt, float grad_scale) {
  const float step_size = lr / bc1;
  const i64 n4 = n >> 2;
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n4; i += (i64)gridDim.x * 256) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 mv = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    float* pp = &pv.x; float* gp = &gv.x; float* mp = &mv.x; float* vp = &vv.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float gg = gp[k] * grad_scale;
      if (weight_decay != 0.f) gg = fmaf(weight_decay, pp[k], gg);
      mp[k] = mp[k] + (gg - mp[k]) * (1.0f - beta1);
      vp[k] = vp[k] * beta2 + (1.0f - beta2) * gg * gg;
      const float denom = sqrtf(vp[k]) / bc2_sqrt + eps;
      pp[k] = pp[k] - step_size * (mp[k] / denom);
    }
    reinterpret_cast<float4*>(p)[i] = pv;
    reinterpret_cast<float4*>(m)[i] = mv;
    reinterpret_cast<float4*>(v)[i] = vv;
  }
  // tail
  for (i64 i = (n4 << 2) + (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
    float gg = g[i] * grad_scale;
    if (weight_decay != 0.f) gg = fmaf(weight_decay, p[i], gg);
    const float mm = m[i] + (gg - m[i]) * (1.0f - beta1);
    const float vv = v[i] * beta2 + (1.0f - beta2) * gg * gg;
    m[i] = mm;
    v[i] = vv;
    p[i] = p[i] - step_size * (mm / (sqrtf(vv) / bc2_sqrt + eps));
  }
}

__global__ __launch_bounds__(256) void adam_step_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ m, float* __restrict__ v, i64 n, float lr,
                                                          float beta1, float beta2, float eps, float weight_decay,
                                                          float bc1, float bc2_sqrt, float grad_scale) {
  adam_step_body(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, grad_scale);
}

// What every update entry checks first: `args_ok`, its own null / range conditions, then the 16-byte alignment that the
// float4 walk needs.  NULL counts as aligned: SGD without momentum has no state buffer.
static int require_update_buffers(const char* entry, bool args_ok, const void* a, const void* b, const void* c,
                                  const void* d) {
  SEG3D_REQUIRE(args_ok, "%s: bad arguments", entry);
  SEG3D_REQUIRE(((uintptr_t)a % 16) == 0 && ((uintptr_t)b % 16) == 0 && ((uintptr_t)c % 16) == 0 && ((uintptr_t)d % 16) == 0,
                "%s: buffers must be 16-byte aligned", entry);
  return SEG3D_OK;
}

// step >= 1 is the 1-based step count AFTER increment (torch increments before use).
// grad_scale multiplies the gradient first (1/world_size after a sum all-reduce; 1.0 otherwise).
extern "C" int seg3d_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n, int step,
                               float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                               void* stream) {
  if (int rc = require_update_buffers("seg3d_adam_step", params && grads && exp_avg && exp_avg_sq && n > 0 && step >= 1,
                                      params, grads, exp_avg, exp_avg_sq))
    return rc;
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  hipLaunchKernelGGL(adam_step_kernel, dim3(seg3d_ew_grid(n / 4 + 1, 256)), dim3(256), 0, (hipStream_t)stream, params, grads,
                     exp_avg, exp_avg_sq, (i64)n, lr, beta1, beta2, eps, weight_decay, (float)bc1, (float)sqrt(bc2),
                     grad_scale);
  SEG3D_LAUNCH_CHECK("seg3d_adam_step");
  return SEG3D_OK;
}

// ---- device-resident control block: gradient-norm clipping, learning-rate schedules, SGD --------------------------
// A train step captured in a hipGraph cannot change a launch argument, and a host read-back of the gradient norm would
// stall the stream: the per-step scalars (learning rate, gradient multiplier, Adam's bias corrections) live in a small
// control block on the device (SEG3D_CTL_* in seg3d_hip.h), written by a one-workgroup prepare kernel and read by the
// update kernels.  A step is: [sum of squares, only when clipping] -> prepare -> update.

// Sum of squares of a flat fp32 buffer: one fp64 slot per workgroup, no atomics.  Each product is exact in fp64 (24-bit x
// 24-bit significands) and everything from the per-thread partial onward is accumulated in fp64, so |g| = 1e30 does not
// overflow.  Grid and traversal are functions of n alone: two calls on the same data give the same bits.
// FusedAdam / FusedSGD pad every parameter to 64 floats; zero_grad() zeroes the whole buffer and no kernel writes the
// padding, so the sum over the flat buffer IS the sum over the parameters.
// HBM-bound: one read of 4 B per element (58 MB for the 14.56 M-parameter V-Net).
__global__ __launch_bounds__(256) void grad_sumsq_partial_kernel(const float* __restrict__ g, i64 n,
                                                                   double* __restrict__ part) {
  __shared__ double red[4];
  double acc = 0.0;
  const i64 n4 = n >> 2;
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n4; i += (i64)gridDim.x * 256) {
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    acc += (double)gv.x * (double)gv.x;
    acc += (double)gv.y * (double)gv.y;
    acc += (double)gv.z * (double)gv.z;
    acc += (double)gv.w * (double)gv.w;
  }
  // tail
  for (i64 i = (n4 << 2) + (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256)
    acc += (double)g[i] * (double)g[i];
  acc = wave_sum_d(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

extern "C" long long seg3d_grad_sumsq_part_count(long long n) { return n > 0 ? seg3d_ew_grid(n / 4 + 1, 256) : 0; }

extern "C" int seg3d_grad_sumsq_partial(const float* grads, long long n, double* part, void* stream) {
  SEG3D_REQUIRE(grads && part && n > 0, "seg3d_grad_sumsq_partial: bad arguments");
  SEG3D_REQUIRE(((uintptr_t)grads % 16) == 0 && ((uintptr_t)part % 8) == 0,
                "seg3d_grad_sumsq_partial: grads must be 16-byte aligned, part 8-byte aligned");
  hipLaunchKernelGGL(grad_sumsq_partial_kernel, dim3((unsigned)seg3d_grad_sumsq_part_count(n)), dim3(256), 0,
                     (hipStream_t)stream, grads, (i64)n, part);
  SEG3D_LAUNCH_CHECK("seg3d_grad_sumsq_partial");
  return SEG3D_OK;
}

// lr of the step that follows s completed steps: base_lr * warm-up * decay, in fp64 (restated by optim/lr_schedule.py)
__device__ __forceinline__ double optim_lr(int s, int schedule, double base_lr, int total_steps, int warmup_steps,
                                           double power) {
  double w = 1.0;
  if (warmup_steps > 0) w = fmin(1.0, ((double)s + 1.0) / (double)warmup_steps);
  double d = 1.0;
  const double T = (double)total_steps;
  if (schedule == SEG3D_SCHEDULE_POLY) {
    d = pow(fmax(0.0, 1.0 - (double)s / T), power);
  } else if (schedule == SEG3D_SCHEDULE_COSINE) {
    d = 0.5 * (1.0 + cos(3.14159265358979323846 * fmin((double)s, T) / T));
  }
  return base_lr * w * d;
}

// One workgroup: adds the nparts sum-of-squares slots (of ALL parameter groups) in a fixed order in fp64, advances *step
// and writes the control block.  The bias corrections are seg3d_adam_step's expressions, evaluated here by the device's
// pow: the same float32 bits for every step count tested (tests/test_gpu_optim.py).
__global__ __launch_bounds__(256) void optim_prepare_kernel(int* __restrict__ step, float* __restrict__ ctl,
                                                              const double* __restrict__ part, int nparts, float grad_scale,
                                                              float max_norm, int schedule, float base_lr, int total_steps,
                                                              int warmup_steps, float power, float beta1, float beta2) {
  __shared__ double red[4];
  double norm = 0.0, coef = 1.0;
  if (max_norm > 0.f) {   // wave-uniform: a launch argument
    double acc = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) acc += part[i];
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      const double sum = ((red[0] + red[1]) + red[2]) + red[3];
      norm = (double)grad_scale * sqrt(sum);
      coef = fmin(1.0, (double)max_norm / (norm + 1e-6));   // torch.nn.utils.clip_grad_norm_ (a NaN norm stays a NaN coef)
      if (norm != norm) coef = norm;
    }
  }
  if (threadIdx.x == 0) {
    const int t = *step + 1;
    *step = t;
    ctl[SEG3D_CTL_LR] = (float)optim_lr(t - 1, schedule, (double)base_lr, total_steps, warmup_steps, (double)power);
    ctl[SEG3D_CTL_GRAD_MULT] = coef == 1.0 ? grad_scale : (float)((double)grad_scale * coef);
    ctl[SEG3D_CTL_BC1] = (float)(1.0 - pow((double)beta1, (double)t));
    ctl[SEG3D_CTL_BC2_SQRT] = (float)sqrt(1.0 - pow((double)beta2, (double)t));
    ctl[SEG3D_CTL_NORM] = (float)norm;
    ctl[SEG3D_CTL_COEF] = (float)coef;
  }
}

extern "C" int seg3d_optim_prepare(int* step_dev, float* ctl, const double* part, int nparts, float grad_scale,
                                   float max_norm, int schedule, float base_lr, int total_steps, int warmup_steps,
                                   float power, float beta1, float beta2, void* stream) {
  SEG3D_REQUIRE(step_dev && ctl, "seg3d_optim_prepare: bad arguments");
  SEG3D_REQUIRE(!(max_norm > 0.f) || (part && nparts > 0), "seg3d_optim_prepare: clipping needs the sum-of-squares slots");
  SEG3D_REQUIRE(schedule >= SEG3D_SCHEDULE_CONSTANT && schedule <= SEG3D_SCHEDULE_COSINE,
                "seg3d_optim_prepare: unknown schedule %d", schedule);
  SEG3D_REQUIRE(total_steps >= 1 && warmup_steps >= 0 && power >= 0.f && base_lr >= 0.f,
                "seg3d_optim_prepare: total_steps >= 1, warmup_steps >= 0, power >= 0, base_lr >= 0 required");
  hipLaunchKernelGGL(optim_prepare_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, step_dev, ctl, part, nparts,
                     grad_scale, max_norm, schedule, base_lr, total_steps, warmup_steps, power, beta1, beta2);
  SEG3D_LAUNCH_CHECK("seg3d_optim_prepare");
  return SEG3D_OK;
}

__global__ __launch_bounds__(256) void adam_step_ctl_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                              float* __restrict__ m, float* __restrict__ v, i64 n,
                                                              const float* __restrict__ ctl, float beta1, float beta2,
                                                              float eps, float weight_decay) {
  adam_step_body(p, g, m, v, n, ctl[SEG3D_CTL_LR], beta1, beta2, eps, weight_decay, ctl[SEG3D_CTL_BC1],
                 ctl[SEG3D_CTL_BC2_SQRT], ctl[SEG3D_CTL_GRAD_MULT]);
}

extern "C" int seg3d_adam_step_ctl(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n,
                                   const float* ctl, float beta1, float beta2, float eps, float weight_decay,
                                   void* stream) {
  if (int rc = require_update_buffers("seg3d_adam_step_ctl", params && grads && exp_avg && exp_avg_sq && n > 0 && ctl,
                                      params, grads, exp_avg, exp_avg_sq))
    return rc;
  hipLaunchKernelGGL(adam_step_ctl_kernel, dim3(seg3d_ew_grid(n / 4 + 1, 256)), dim3(256), 0, (hipStream_t)stream, params,
                     grads, exp_avg, exp_avg_sq, (i64)n, ctl, beta1, beta2, eps, weight_decay);
  SEG3D_LAUNCH_CHECK("seg3d_adam_step_ctl");
  return SEG3D_OK;
}

// torch.optim.SGD (dampening 0), single-tensor path restated:
//   g += wd * p;  buf = mu * buf + g;  d = nesterov ? g + mu * buf : buf;  p -= lr * d
// torch's first step sets buf = g, which is what a zero-initialised buf gives.  MOM = false (mu == 0): buf is neither
// read nor written and d = g.  HBM-bound: 3 reads + 2 writes of 4 B per parameter (20 B/param), 2 + 1 without momentum.
template <bool MOM, bool NEST>
__device__ __forceinline__ float sgd_update(float p, float g, float* buf, float mult, float lr, float mu, float wd) {
  float gg = g * mult;
  if (wd != 0.f) gg = fmaf(wd, p, gg);
  float d = gg;
  if (MOM) {
    const float b = mu * *buf + gg;
    *buf = b;
    d = NEST ? gg + mu * b : b;
  }
  return p - lr * d;
}

template <bool MOM, bool NEST>
__global__ __launch_bounds__(256) void sgd_step_ctl_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                             float* __restrict__ buf, i64 n, const float* __restrict__ ctl,
                                                             float mu, float wd) {
  const float lr = ctl[SEG3D_CTL_LR], mult = ctl[SEG3D_CTL_GRAD_MULT];
  const i64 n4 = n >> 2;
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n4; i += (i64)gridDim.x * 256) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (MOM) bv = reinterpret_cast<float4*>(buf)[i];
    float* pp = &pv.x; const float* gp = &gv.x; float* bp = &bv.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) pp[k] = sgd_update<MOM, NEST>(pp[k], gp[k], &bp[k], mult, lr, mu, wd);
    reinterpret_cast<float4*>(p)[i] = pv;
    if (MOM) reinterpret_cast<float4*>(buf)[i] = bv;
  }
  // tail
  for (i64 i = (n4 << 2) + (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
    float b = MOM ? buf[i] : 0.f;
    p[i] = sgd_update<MOM, NEST>(p[i], g[i], &b, mult, lr, mu, wd);
    if (MOM) buf[i] = b;
  }
}

extern "C" int seg3d_sgd_step_ctl(float* params, const float* grads, float* momentum_buf, long long n, const float* ctl,
                                  float momentum, float weight_decay, int nesterov, void* stream) {
  if (int rc = require_update_buffers("seg3d_sgd_step_ctl", params && grads && n > 0 && ctl, params, grads, momentum_buf,
                                      nullptr))
    return rc;
  SEG3D_REQUIRE(momentum >= 0.f && (momentum == 0.f || momentum_buf), "seg3d_sgd_step_ctl: momentum needs its buffer");
  SEG3D_REQUIRE(!nesterov || momentum > 0.f, "seg3d_sgd_step_ctl: Nesterov needs momentum > 0");
  const dim3 grid(seg3d_ew_grid(n / 4 + 1, 256)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (momentum == 0.f)
    hipLaunchKernelGGL((sgd_step_ctl_kernel<false, false>), grid, block, 0, s, params, grads, momentum_buf, (i64)n, ctl,
                       momentum, weight_decay);
  else if (nesterov)
    hipLaunchKernelGGL((sgd_step_ctl_kernel<true, true>), grid, block, 0, s, params, grads, momentum_buf, (i64)n, ctl,
                       momentum, weight_decay);
  else
    hipLaunchKernelGGL((sgd_step_ctl_kernel<true, false>), grid, block, 0, s, params, grads, momentum_buf, (i64)n, ctl,
                       momentum, weight_decay);
  SEG3D_LAUNCH_CHECK("seg3d_sgd_step_ctl");
  return SEG3D_OK;
}
