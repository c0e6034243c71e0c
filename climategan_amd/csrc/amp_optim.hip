// Adam / RMSprop (torch.optim, the reference's get_optimizer, climategan/optim.py:110-121) and the loss-scaling path of
// ``train.amp`` (trainer.py:116-126, 1004-1009, 1020-1025), fused over all parameter tensors.  Three launches per optimizer
// step, none of which the host waits for:
//   check   every gradient element read once; a device flag becomes 1.0f if any is +-inf / NaN (GradScaler's found_inf);
//           with write_back also g = g * inv_scale (GradScaler.unscale_).  4 B per element, nothing written without it.
//   update  returns untouched when the flag is set; otherwise g' = g * inv_scale (in registers: p.grad stays scaled) and
//           Adam     g' += wd p ; m = b1 m + (1-b1) g' ; v = b2 v + (1-b2) g'^2
//                    p -= (lr / (1-b1^t)) m / (sqrt(v) / sqrt(1-b2^t) + eps)              16 B read + 12 B written / element
//           RMSprop  g' += wd p ; v = a v + (1-a) g'^2 ; p -= lr g' / (sqrt(v) + eps)     12 B read +  8 B written / element
//           t = *step + 1: the per-parameter step count lives on the device (the skip is decided there), the two bias
//           corrections are formed from it in double once per block.
//   finish  *step += 1 for every tensor of the table unless the flag is set.
// HBM-bound element-wise work, every byte touched once per launch: non-temporal accesses, four elements per thread where the
// tensors' addresses allow 16-byte accesses.
#include <math.h>

#include "cgan_common.h"

namespace {

__device__ __forceinline__ bool nonfinite(float x) { return (__builtin_bit_cast(uint32_t, x) & 0x7f800000u) == 0x7f800000u; }

__device__ __forceinline__ bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr,
                                          const void* d = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15u) == 0;
}

__global__ __launch_bounds__(256) void grads_nonfinite_check_kernel(const CganAmpOptimItem* __restrict__ items,
                                                                    float inv_scale, int write_back,
                                                                    float* __restrict__ found_inf) {
  const CganAmpOptimItem it = items[blockIdx.y];
  const long n = it.numel;
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
  bool bad = false;
  long done = 0;
  if (aligned16(it.g)) {
    const long n4 = n >> 2;
    f32x4* g4 = reinterpret_cast<f32x4*>(it.g);
    for (long i = tid; i < n4; i += nth) {
      f32x4 g = CGAN_LD_STREAM(g4 + i);
      bad = bad || nonfinite(g.x) || nonfinite(g.y) || nonfinite(g.z) || nonfinite(g.w);
      if (write_back) {
        g.x *= inv_scale, g.y *= inv_scale, g.z *= inv_scale, g.w *= inv_scale;
        CGAN_ST_STREAM(g, g4 + i);
      }
    }
    done = n4 << 2;
  }
  for (long i = done + tid; i < n; i += nth) {          // the tail (at most 3 elements), or a tensor at an odd address
    const float g = CGAN_LD_STREAM(it.g + i);
    bad = bad || nonfinite(g);
    if (write_back) CGAN_ST_STREAM(g * inv_scale, it.g + i);
  }
  // a plain store of the same value from every thread that saw one: no read-modify-write, no same-address atomic
  if (bad) *found_inf = 1.0f;
}

struct UpdateArgs {
  double lr, beta1, beta2, eps, weight_decay;
  float inv_scale;
  int rmsprop;
};

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float inv_scale, float wd, float beta1,
                                         float omb1, float beta2, float omb2, float step_size, float bc2_sqrt, float eps) {
  g *= inv_scale;
  if (wd != 0.f) g = g + wd * p;
  m = m * beta1 + omb1 * g;
  v = v * beta2 + omb2 * g * g;
  const float denom = sqrtf(v) / bc2_sqrt + eps;
  p = p - step_size * m / denom;
}

__device__ __forceinline__ void rmsprop_one(float& p, float g, float& v, float inv_scale, float wd, float alpha, float oma,
                                            float lr, float eps) {
  g *= inv_scale;
  if (wd != 0.f) g = g + wd * p;
  v = v * alpha + oma * g * g;
  p = p - lr * g / (sqrtf(v) + eps);
}

template <bool RMSPROP>
__global__ __launch_bounds__(256) void amp_optim_update_kernel(const CganAmpOptimItem* __restrict__ items, UpdateArgs a,
                                                               const float* __restrict__ found_inf) {
  if (found_inf && *found_inf != 0.f) return;           // a skipped step writes nothing (uniform over the whole grid)
  const CganAmpOptimItem it = items[blockIdx.y];
  const long n = it.numel;
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
  if ((long)blockIdx.x * blockDim.x >= n) return;       // uniform per block: nothing of this tensor falls to it
  __shared__ float s_corr[2];
  if (!RMSPROP) {
    if (threadIdx.x == 0) {
      // torch.optim.Adam: bias_correction = 1 - beta ** step in Python floats, step counted from 1
      const double t = (double)*it.step + 1.0;
      const double bc1 = 1.0 - pow(a.beta1, t), bc2 = 1.0 - pow(a.beta2, t);
      s_corr[0] = (float)(a.lr / bc1);
      s_corr[1] = (float)sqrt(bc2);
    }
    __syncthreads();
  }
  const float step_size = RMSPROP ? (float)a.lr : s_corr[0], bc2_sqrt = RMSPROP ? 1.f : s_corr[1];
  const float beta1 = (float)a.beta1, omb1 = (float)(1.0 - a.beta1), beta2 = (float)a.beta2, omb2 = (float)(1.0 - a.beta2);
  const float eps = (float)a.eps, wd = (float)a.weight_decay, inv_scale = a.inv_scale;
  long done = 0;
  if (aligned16(it.p, it.g, it.m, it.v)) {
    const long n4 = n >> 2;
    f32x4* p4 = reinterpret_cast<f32x4*>(it.p);
    const f32x4* g4 = reinterpret_cast<const f32x4*>(it.g);
    f32x4* m4 = reinterpret_cast<f32x4*>(it.m);
    f32x4* v4 = reinterpret_cast<f32x4*>(it.v);
    for (long i = tid; i < n4; i += nth) {
      const f32x4 pv = CGAN_LD_STREAM(p4 + i), gv = CGAN_LD_STREAM(g4 + i), vv = CGAN_LD_STREAM(v4 + i);
      float p[4] = {pv.x, pv.y, pv.z, pv.w}, v[4] = {vv.x, vv.y, vv.z, vv.w};
      const float g[4] = {gv.x, gv.y, gv.z, gv.w};
      if (RMSPROP) {
#pragma unroll
        for (int k = 0; k < 4; ++k) rmsprop_one(p[k], g[k], v[k], inv_scale, wd, beta2, omb2, step_size, eps);
      } else {
        const f32x4 mv = CGAN_LD_STREAM(m4 + i);
        float m[4] = {mv.x, mv.y, mv.z, mv.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
          adam_one(p[k], g[k], m[k], v[k], inv_scale, wd, beta1, omb1, beta2, omb2, step_size, bc2_sqrt, eps);
        const f32x4 mo = {m[0], m[1], m[2], m[3]};
        CGAN_ST_STREAM(mo, m4 + i);
      }
      const f32x4 vo = {v[0], v[1], v[2], v[3]}, po = {p[0], p[1], p[2], p[3]};
      CGAN_ST_STREAM(vo, v4 + i);
      CGAN_ST_STREAM(po, p4 + i);
    }
    done = n4 << 2;
  }
  for (long i = done + tid; i < n; i += nth) {
    float p = it.p[i], v = it.v[i];
    const float g = it.g[i];
    if (RMSPROP) {
      rmsprop_one(p, g, v, inv_scale, wd, beta2, omb2, step_size, eps);
    } else {
      float m = it.m[i];
      adam_one(p, g, m, v, inv_scale, wd, beta1, omb1, beta2, omb2, step_size, bc2_sqrt, eps);
      it.m[i] = m;
    }
    it.v[i] = v;
    it.p[i] = p;
  }
}

__global__ __launch_bounds__(256) void amp_optim_finish_kernel(const CganAmpOptimItem* __restrict__ items, int count,
                                                               const float* __restrict__ found_inf) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  if (found_inf && *found_inf != 0.f) return;
  float* step = items[i].step;
  *step = *step + 1.0f;
}

// four elements per thread, at most 1024 blocks per tensor (the grid-stride loop takes the rest)
unsigned blocks_for(int64_t max_numel) {
  long blocks = (max_numel + 1023) / 1024;
  return (unsigned)(blocks > 1024 ? 1024 : blocks);
}

}  // namespace

extern "C" int cgan_grads_nonfinite_check_multi_tensor(const CganAmpOptimItem* items_device, int32_t count,
                                                       int64_t max_numel, double inv_scale, int32_t write_back,
                                                       float* found_inf_device, void* stream) {
  CGAN_REQUIRE(items_device && count > 0 && count <= 65535 && max_numel > 0, "grads_nonfinite_check: bad arguments");
  CGAN_REQUIRE(found_inf_device, "grads_nonfinite_check: found_inf_device is null");
  CGAN_REQUIRE(write_back == 0 || write_back == 1, "grads_nonfinite_check: write_back must be 0 or 1");
  CGAN_REQUIRE(isfinite(inv_scale) && inv_scale > 0., "grads_nonfinite_check: inv_scale must be positive and finite");
  hipLaunchKernelGGL(grads_nonfinite_check_kernel, dim3(blocks_for(max_numel), count), dim3(256), 0, (hipStream_t)stream,
                     items_device, (float)inv_scale, write_back, found_inf_device);
  CGAN_CHECK_LAUNCH("grads_nonfinite_check_multi_tensor");
  return CGAN_OK;
}

static int launch_update(const CganAmpOptimItem* items_device, int32_t count, int64_t max_numel, const UpdateArgs& a,
                         const float* found_inf_device, void* stream, const char* name) {
  const dim3 grid(blocks_for(max_numel), count);
  if (a.rmsprop)
    hipLaunchKernelGGL(amp_optim_update_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, items_device, a,
                       found_inf_device);
  else
    hipLaunchKernelGGL(amp_optim_update_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, items_device, a,
                       found_inf_device);
  CGAN_CHECK_LAUNCH(name);
  return CGAN_OK;
}

extern "C" int cgan_adam_multi_tensor(const CganAmpOptimItem* items_device, int32_t count, int64_t max_numel, double lr,
                                      double beta1, double beta2, double eps, double weight_decay, double inv_scale,
                                      const float* found_inf_device, void* stream) {
  CGAN_REQUIRE(items_device && count > 0 && count <= 65535 && max_numel > 0, "adam: bad arguments");
  CGAN_REQUIRE(lr >= 0. && eps >= 0. && beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1. && weight_decay >= 0.,
               "adam: Invalid hyper-parameter");
  CGAN_REQUIRE(isfinite(inv_scale) && inv_scale > 0., "adam: inv_scale must be positive and finite");
  const UpdateArgs a = {lr, beta1, beta2, eps, weight_decay, (float)inv_scale, 0};
  return launch_update(items_device, count, max_numel, a, found_inf_device, stream, "adam_multi_tensor");
}

extern "C" int cgan_rmsprop_multi_tensor(const CganAmpOptimItem* items_device, int32_t count, int64_t max_numel, double lr,
                                         double alpha, double eps, double weight_decay, double inv_scale,
                                         const float* found_inf_device, void* stream) {
  CGAN_REQUIRE(items_device && count > 0 && count <= 65535 && max_numel > 0, "rmsprop: bad arguments");
  CGAN_REQUIRE(lr >= 0. && eps >= 0. && alpha >= 0. && weight_decay >= 0., "rmsprop: Invalid hyper-parameter");
  CGAN_REQUIRE(isfinite(inv_scale) && inv_scale > 0., "rmsprop: inv_scale must be positive and finite");
  const UpdateArgs a = {lr, 0., alpha, eps, weight_decay, (float)inv_scale, 1};     // beta2 carries alpha
  return launch_update(items_device, count, max_numel, a, found_inf_device, stream, "rmsprop_multi_tensor");
}

extern "C" int cgan_amp_optim_finish(const CganAmpOptimItem* items_device, int32_t count, const float* found_inf_device,
                                     void* stream) {
  CGAN_REQUIRE(items_device && count > 0, "amp_optim_finish: bad arguments");
  hipLaunchKernelGGL(amp_optim_finish_kernel, dim3((count + 255) / 256), dim3(256), 0, (hipStream_t)stream, items_device,
                     count, found_inf_device);
  CGAN_CHECK_LAUNCH("amp_optim_finish");
  return CGAN_OK;
}
