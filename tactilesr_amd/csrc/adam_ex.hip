// The Adam family beyond the reference's choice in ONE launch over a chunk table: decoupled weight decay
// (torch.optim.AdamW) and AMSGrad, tsr_adam_multi_ex / tsr_adam_multi_ex_dev (include/tactilesr_hip.h).  The launch
// shape is the legacy fused step's (train_ops.hip, adam_l2_multi_body): block b owns chunk record b, <= 4096 contiguous
// elements of one tensor, and the moment updates are written as that body writes them (here with every operation
// rounded on its own: no compiler-chosen multiply-adds).  Bandwidth-bound: seven tensor
// passes (p, m, v read and written, g read), nine with AMSGrad, one more when a clipped gradient is written back.
#include <math.h>
#include "tsr_common.h"
#include "tactilesr_hip.h"

#define ADAM_EX_FLAGS (TSR_ADAM_DECOUPLED | TSR_ADAM_AMSGRAD)

struct adam_ex_args {      // the per-launch scalars; h = {lr, bc1, bc2_sqrt, decay}
  float b1, b2, omb1, omb2, eps, wd;
};

// FLAGS and CLIP are compile-time per instantiation; the kernels below pick the instantiation from the (workgroup-
// uniform) runtime flags.  vmax is read only with AMSGRAD.
template <int FLAGS, bool CLIP>
__device__ __forceinline__ void adam_ex_body(const tsr_adam_chunk* __restrict__ chunks, float* const* __restrict__ vmax,
                                             const adam_ex_args a, float lr, float bc1, float bc2_sqrt, float decay,
                                             const float* __restrict__ clip) {
  constexpr bool DEC = (FLAGS & TSR_ADAM_DECOUPLED) != 0;
  constexpr bool AMS = (FLAGS & TSR_ADAM_AMSGRAD) != 0;
  const tsr_adam_chunk c = chunks[blockIdx.x];
  if (c.n < 1 || c.n > 4096) return;                  // a bad record: nothing read, nothing written
  float* vm_p = nullptr;
  if (AMS) vm_p = vmax[blockIdx.x];
  const float step_size = lr / bc1;
  const float b1 = a.b1, b2 = a.b2, omb1 = a.omb1, omb2 = a.omb2, eps = a.eps, wd = a.wd;
  auto upd = [&](float w, float g, float& m, float& v, float& vm) {
    // Every operation rounds on its own (the one fmaf is written out): left to the compiler, which products fuse into
    // multiply-adds differs between the instantiations, and the forms must agree bit for bit where the formulas do
    // (weight_decay = 0: DECOUPLED and L2; the vector and the scalar path).
#pragma clang fp contract(off)
    float gg, w0;
    if (DEC) {
      gg = g;
      w0 = __fmul_rn(w, decay);
    } else {
      gg = fmaf(wd, w, g);
      w0 = w;
    }
    m = b1 * m + omb1 * gg;
    v = b2 * v + omb2 * gg * gg;
    float vhat = v;
    if (AMS) {
      vm = (v != v || vm != vm) ? (v + vm) : (vm > v ? vm : v);      // torch.maximum: a NaN propagates
      vhat = vm;
    }
    return w0 - step_size * (m / (sqrtf(vhat) / bc2_sqrt + eps));
  };
  float coef = 1.0f;
  if (CLIP) coef = clip[0];
  // coef == 1 multiplies exactly: the gradient already holds the clipped value (NaN != 1: a NaN coefficient writes)
  const bool write_grad = CLIP && !(coef == 1.0f);
  float* grad_out = const_cast<float*>(c.grad);
  const bool vec = ((((size_t)c.param | (size_t)c.grad | (size_t)c.exp_avg | (size_t)c.exp_avg_sq | (size_t)vm_p) & 15) == 0);
  const int n4 = vec ? (c.n >> 2) : 0;
  for (int i = threadIdx.x; i < n4; i += 256) {
    f32x4 w = ((f32x4*)c.param)[i], m = ((f32x4*)c.exp_avg)[i], v = ((f32x4*)c.exp_avg_sq)[i];
    f32x4 g = ((const f32x4*)c.grad)[i];
    f32x4 vm = {0.f, 0.f, 0.f, 0.f};
    if (AMS) vm = ((f32x4*)vm_p)[i];
    if (CLIP) {
#pragma unroll
      for (int j = 0; j < 4; ++j) g[j] = __fmul_rn(g[j], coef);
      if (write_grad) ((f32x4*)grad_out)[i] = g;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float mj = m[j], vj = v[j], vmj = vm[j];
      w[j] = upd(w[j], g[j], mj, vj, vmj);
      m[j] = mj;
      v[j] = vj;
      vm[j] = vmj;
    }
    ((f32x4*)c.param)[i] = w;
    ((f32x4*)c.exp_avg)[i] = m;
    ((f32x4*)c.exp_avg_sq)[i] = v;
    if (AMS) ((f32x4*)vm_p)[i] = vm;
  }
  for (int i = n4 * 4 + threadIdx.x; i < c.n; i += 256) {
    float m = c.exp_avg[i], v = c.exp_avg_sq[i], vm = 0.f;
    float g = c.grad[i];
    if (AMS) vm = vm_p[i];
    if (CLIP) {
      g = __fmul_rn(g, coef);
      if (write_grad) grad_out[i] = g;
    }
    c.param[i] = upd(c.param[i], g, m, v, vm);
    c.exp_avg[i] = m;
    c.exp_avg_sq[i] = v;
    if (AMS) vm_p[i] = vm;
  }
}

template <bool CLIP>
__device__ __forceinline__ void adam_ex_pick(const tsr_adam_chunk* __restrict__ chunks, float* const* __restrict__ vmax,
                                             int flags, const adam_ex_args a, float lr, float bc1, float bc2_sqrt,
                                             float decay, const float* __restrict__ clip) {
  switch (flags) {
    case 0: adam_ex_body<0, CLIP>(chunks, vmax, a, lr, bc1, bc2_sqrt, decay, clip); break;
    case TSR_ADAM_DECOUPLED: adam_ex_body<TSR_ADAM_DECOUPLED, CLIP>(chunks, vmax, a, lr, bc1, bc2_sqrt, decay, clip); break;
    case TSR_ADAM_AMSGRAD: adam_ex_body<TSR_ADAM_AMSGRAD, CLIP>(chunks, vmax, a, lr, bc1, bc2_sqrt, decay, clip); break;
    case ADAM_EX_FLAGS: adam_ex_body<ADAM_EX_FLAGS, CLIP>(chunks, vmax, a, lr, bc1, bc2_sqrt, decay, clip); break;
    default: break;
  }
}

__global__ __launch_bounds__(256) void adam_ex_kernel(const tsr_adam_chunk* __restrict__ chunks,
                                                      float* const* __restrict__ vmax, int flags, adam_ex_args a,
                                                      float lr, float bc1, float bc2_sqrt, float decay) {
  adam_ex_pick<false>(chunks, vmax, flags, a, lr, bc1, bc2_sqrt, decay, nullptr);
}

// hyper = {lr, bc1, bc2_sqrt, decay} in device memory: a captured graph replays this launch with the values written
// before each replay instead of the ones of the capture.
__global__ __launch_bounds__(256) void adam_ex_dev_kernel(const tsr_adam_chunk* __restrict__ chunks,
                                                          float* const* __restrict__ vmax, int flags, adam_ex_args a,
                                                          const float* __restrict__ hyper) {
  adam_ex_pick<false>(chunks, vmax, flags, a, hyper[0], hyper[1], hyper[2], hyper[3], nullptr);
}

// The clipping forms of the two kernels above: clip[0] is the coefficient tsr_grad_norm_multi wrote.
__global__ __launch_bounds__(256) void adam_ex_clip_kernel(const tsr_adam_chunk* __restrict__ chunks,
                                                           float* const* __restrict__ vmax, int flags, adam_ex_args a,
                                                           float lr, float bc1, float bc2_sqrt, float decay,
                                                           const float* __restrict__ clip) {
  adam_ex_pick<true>(chunks, vmax, flags, a, lr, bc1, bc2_sqrt, decay, clip);
}

__global__ __launch_bounds__(256) void adam_ex_dev_clip_kernel(const tsr_adam_chunk* __restrict__ chunks,
                                                               float* const* __restrict__ vmax, int flags,
                                                               adam_ex_args a, const float* __restrict__ hyper,
                                                               const float* __restrict__ clip) {
  adam_ex_pick<true>(chunks, vmax, flags, a, hyper[0], hyper[1], hyper[2], hyper[3], clip);
}

static bool adam_ex_scalars_bad(double beta1, double beta2, float eps, float weight_decay) {
  return !(eps >= 0.f) || !(weight_decay >= 0.f) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0);
}

static bool adam_ex_table_bad(const tsr_adam_chunk* chunks, float* const* vmax, int n_chunks, int flags) {
  return !chunks || n_chunks <= 0 || (flags & ~ADAM_EX_FLAGS) || ((flags & TSR_ADAM_AMSGRAD) != 0) != (vmax != nullptr);
}

// betas arrive as doubles and every derived constant is formed in double, as in the legacy launches
static adam_ex_args adam_ex_pack(double beta1, double beta2, float eps, float weight_decay) {
  return {(float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, weight_decay};
}

extern "C" int tsr_adam_hyper_ex(float lr, double beta1, double beta2, int step, float weight_decay, int flags,
                                 float* out4) {
#pragma clang fp contract(off)      // the product is rounded on its own, as Python's 1 - lr * weight_decay is
  if (!out4 || step <= 0 || (flags & ~ADAM_EX_FLAGS) || !(lr >= 0.f) || adam_ex_scalars_bad(beta1, beta2, 0.f, weight_decay))
    return TSR_ERR_ARG;
  if (tsr_adam_hyper(lr, beta1, beta2, step, out4) != TSR_OK) return TSR_ERR_ARG;      // the legacy floats, bit for bit
  const double prod = (double)lr * (double)weight_decay;
  out4[3] = (flags & TSR_ADAM_DECOUPLED) ? (float)(1.0 - prod) : 1.0f;
  return TSR_OK;
}

extern "C" int tsr_adam_multi_ex(const tsr_adam_chunk* chunks, float* const* vmax, int n_chunks, int flags, float lr,
                                 double beta1, double beta2, float eps, float weight_decay, int step, const float* clip,
                                 void* stream) {
  if (adam_ex_table_bad(chunks, vmax, n_chunks, flags) || step <= 0 || !(lr >= 0.f) ||
      adam_ex_scalars_bad(beta1, beta2, eps, weight_decay))
    return TSR_ERR_ARG;
  float h[4];
  if (tsr_adam_hyper_ex(lr, beta1, beta2, step, weight_decay, flags, h) != TSR_OK) return TSR_ERR_ARG;
  const adam_ex_args a = adam_ex_pack(beta1, beta2, eps, weight_decay);
  if (clip)
    hipLaunchKernelGGL(adam_ex_clip_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, chunks, vmax, flags, a,
                       h[0], h[1], h[2], h[3], clip);
  else
    hipLaunchKernelGGL(adam_ex_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, chunks, vmax, flags, a, h[0],
                       h[1], h[2], h[3]);
  return tsr_check_launch();
}

extern "C" int tsr_adam_multi_ex_dev(const tsr_adam_chunk* chunks, float* const* vmax, int n_chunks, int flags,
                                     const float* hyper4, double beta1, double beta2, float eps, float weight_decay,
                                     const float* clip, void* stream) {
  if (adam_ex_table_bad(chunks, vmax, n_chunks, flags) || !hyper4 || adam_ex_scalars_bad(beta1, beta2, eps, weight_decay))
    return TSR_ERR_ARG;
  const adam_ex_args a = adam_ex_pack(beta1, beta2, eps, weight_decay);
  if (clip)
    hipLaunchKernelGGL(adam_ex_dev_clip_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, chunks, vmax, flags,
                       a, hyper4, clip);
  else
    hipLaunchKernelGGL(adam_ex_dev_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, chunks, vmax, flags, a,
                       hyper4);
  return tsr_check_launch();
}
