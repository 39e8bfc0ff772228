// Training-path kernels around the MFMA convolutions (all HBM-bound or tiny):
//   BatchNorm2d train mode (batch statistics + running-stat update, backward coefficients),
//   the 3->64 stem and 128->1 head backward, target preparation, MSE loss fwd/bwd, Adam(L2).
// Reference semantics: nn.BatchNorm2d(eps=1e-5, momentum=0.1) inside model/tactileSR_model.py:
// 38-49,167-189; nn.MSELoss + HR/10 + F.interpolate of train/tactileSR_train.py:39-49;
// optim.Adam(lr, weight_decay) (L2-in-grad) of train/tactileSR_train.py:212; the step order of
// cpu/trainer.py:346-362.
#include "tsr_common.h"
#include "tactilesr_hip.h"

#define RED_BLOCKS 512     // partial-sum blocks of the slab reductions (work buffers hold RED_BLOCKS*C*3 doubles)

// ------------------------------------------------------------------------------------------
// per-channel fp64 reduction of the conv epilogue slabs: slab[entry][C][2]
//   mode 0 (Welford partials mean,M2 with counts): S0 = sum n, S1 = sum n*mean, S2 = sum (M2 + n*mean^2)
//   mode 1 (plain sums s1,s2):                      S0 = entries, S1 = sum s1, S2 = sum s2
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void slab_reduce_kernel(const float* __restrict__ slab,
                                                          const float* __restrict__ cnt, int entries, int C,
                                                          int mode, double* __restrict__ part) {
  __shared__ double sh[256 * 3];
  const int tid = threadIdx.x;
  const int per = 256 / C;           // entries handled concurrently by one block (C in {64,128})
  const int c = tid % C, el = tid / C;
  double s0 = 0, s1 = 0, s2 = 0, t0 = 0, t1 = 0, t2 = 0;     // two independent chains: two loads in flight
  const int stride = gridDim.x * per;
  int e = blockIdx.x * per + el;
  for (; e + stride < entries; e += 2 * stride) {
    const float2 v = *(const float2*)(slab + ((size_t)e * C + c) * 2);
    const float2 u = *(const float2*)(slab + ((size_t)(e + stride) * C + c) * 2);
    if (mode == 0) {
      const double n = (double)cnt[e], m = (double)v.x, n2 = (double)cnt[e + stride], m2 = (double)u.x;
      s0 += n; s1 += n * m; s2 += (double)v.y + n * m * m;
      t0 += n2; t1 += n2 * m2; t2 += (double)u.y + n2 * m2 * m2;
    } else {
      s0 += 1.0; s1 += (double)v.x; s2 += (double)v.y;
      t0 += 1.0; t1 += (double)u.x; t2 += (double)u.y;
    }
  }
  if (e < entries) {
    const float2 v = *(const float2*)(slab + ((size_t)e * C + c) * 2);
    if (mode == 0) {
      const double n = (double)cnt[e], m = (double)v.x;
      s0 += n; s1 += n * m; s2 += (double)v.y + n * m * m;
    } else {
      s0 += 1.0; s1 += (double)v.x; s2 += (double)v.y;
    }
  }
  s0 += t0; s1 += t1; s2 += t2;
  sh[tid * 3 + 0] = s0; sh[tid * 3 + 1] = s1; sh[tid * 3 + 2] = s2;
  __syncthreads();
  if (el == 0) {
    for (int k = 1; k < per; ++k) {
      s0 += sh[(k * C + c) * 3 + 0]; s1 += sh[(k * C + c) * 3 + 1]; s2 += sh[(k * C + c) * 3 + 2];
    }
    double* p = part + ((size_t)blockIdx.x * C + c) * 3;
    p[0] = s0; p[1] = s1; p[2] = s2;
  }
}

__global__ void bn_stats_final_kernel(const double* __restrict__ part, int nblocks, int C,
                                      const float* __restrict__ bias, const float* __restrict__ gamma,
                                      const float* __restrict__ beta, float* __restrict__ running_mean,
                                      float* __restrict__ running_var, float momentum, float eps,
                                      float* __restrict__ scale, float* __restrict__ shift,
                                      float* __restrict__ xa, float* __restrict__ xb) {
  // 16 channels per block; 16 lanes per channel walk the partial blocks, then one lane finishes
  __shared__ double sh[256 * 3];
  const int tid = threadIdx.x, cl = tid & 15, kl = tid >> 4;
  const int c = blockIdx.x * 16 + cl;
  double n = 0, s1 = 0, s2 = 0;
  for (int k = kl; k < nblocks; k += 16) {
    const double* p = part + ((size_t)k * C + c) * 3;
    n += p[0]; s1 += p[1]; s2 += p[2];
  }
  sh[tid * 3 + 0] = n; sh[tid * 3 + 1] = s1; sh[tid * 3 + 2] = s2;
  __syncthreads();
  if (kl != 0) return;
  for (int k = 1; k < 16; ++k) {
    n += sh[(k * 16 + cl) * 3 + 0]; s1 += sh[(k * 16 + cl) * 3 + 1]; s2 += sh[(k * 16 + cl) * 3 + 2];
  }
  const double mean = s1 / n;
  double var = s2 / n - mean * mean;          // biased (normalisation)
  var = var < 0 ? 0 : var;
  const double invstd = 1.0 / sqrt(var + (double)eps);
  const double sc = (double)gamma[c] * invstd;
  scale[c] = (float)sc;
  shift[c] = (float)((double)beta[c] - mean * sc);
  xa[c] = (float)invstd;
  xb[c] = (float)(-mean * invstd);
  if (running_mean) {
    const double mz = mean + (bias ? (double)bias[c] : 0.0);   // stats were taken on the bias-free accumulator
    const double unbiased = n > 1 ? var * n / (n - 1) : var;
    running_mean[c] = (float)((1.0 - momentum) * running_mean[c] + momentum * mz);
    running_var[c] = (float)((1.0 - momentum) * running_var[c] + momentum * unbiased);
  }
}

extern "C" int tsr_bn_stats_finalize(const float* slab, const float* slab_cnt, int entries, int C,
                                     const float* bias, const float* gamma, const float* beta,
                                     float* running_mean, float* running_var, float momentum, float eps,
                                     float* scale, float* shift, float* xhat_a, float* xhat_b,
                                     double* work, void* stream) {
  if (!slab || !slab_cnt || !gamma || !beta || !scale || !shift || !xhat_a || !xhat_b || !work || entries <= 0 ||
      (C != 64 && C != 128))
    return TSR_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(slab_reduce_kernel, dim3(RED_BLOCKS), dim3(256), 0, st, slab, slab_cnt, entries, C, 0, work);
  hipLaunchKernelGGL(bn_stats_final_kernel, dim3(C / 16), dim3(256), 0, st, work, RED_BLOCKS, C, bias, gamma, beta,
                     running_mean, running_var, momentum, eps, scale, shift, xhat_a, xhat_b);
  return tsr_check_launch();
}

__global__ void bn_bwd_final_kernel(const double* __restrict__ part, int nblocks, int C, double N,
                                    const float* __restrict__ scale, const float* __restrict__ xa,
                                    const float* __restrict__ xb, float* __restrict__ dgamma,
                                    float* __restrict__ dbeta, float* __restrict__ c1, float* __restrict__ c2,
                                    float* __restrict__ c3) {
  __shared__ double sh[256 * 2];
  const int tid = threadIdx.x, cl = tid & 15, kl = tid >> 4;
  const int c = blockIdx.x * 16 + cl;
  double s1 = 0, s2 = 0;
  for (int k = kl; k < nblocks; k += 16) {
    const double* p = part + ((size_t)k * C + c) * 3;
    s1 += p[1]; s2 += p[2];
  }
  sh[tid * 2 + 0] = s1; sh[tid * 2 + 1] = s2;
  __syncthreads();
  if (kl != 0) return;
  for (int k = 1; k < 16; ++k) { s1 += sh[(k * 16 + cl) * 2 + 0]; s2 += sh[(k * 16 + cl) * 2 + 1]; }
  dbeta[c] = (float)s1;
  dgamma[c] = (float)s2;
  // dz = scale*(g - dbeta/N - xhat*dgamma/N), xhat = z*xa + xb  ->  dz = c1*g + c2*z + c3
  const double sc = scale[c];
  c1[c] = (float)sc;
  c2[c] = (float)(-sc * s2 / N * (double)xa[c]);
  c3[c] = (float)(-sc * (s1 / N + (double)xb[c] * s2 / N));
}

extern "C" int tsr_bn_bwd_finalize(const float* slab, int entries, int C, double N, const float* scale,
                                   const float* xhat_a, const float* xhat_b, float* dgamma, float* dbeta,
                                   float* c1, float* c2, float* c3, double* work, void* stream) {
  if (!slab || !scale || !xhat_a || !xhat_b || !dgamma || !dbeta || !c1 || !c2 || !c3 || !work || entries <= 0 ||
      (C != 64 && C != 128))
    return TSR_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(slab_reduce_kernel, dim3(RED_BLOCKS), dim3(256), 0, st, slab, (const float*)nullptr, entries,
                     C, 1, work);
  hipLaunchKernelGGL(bn_bwd_final_kernel, dim3(C / 16), dim3(256), 0, st, work, RED_BLOCKS, C, N, scale, xhat_a, xhat_b,
                     dgamma, dbeta, c1, c2, c3);
  return tsr_check_launch();
}

// g[:, gcoff:gcoff+C] = c1*g + c2*z[:, zcoff:zcoff+C] + c3   (BN backward, elementwise, CB16, in place)
// One workgroup per (image, 16-channel block): its HW x 16 values are contiguous; a thread keeps one channel quad (c1..c3 in
// 12 registers, no index arithmetic per element) and has UNR independent 16-B load pairs in flight.
template <bool B16>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(float* __restrict__ g, int g_ctot, int g_coff,
                                                           const float* __restrict__ z, int z_ctot, int z_coff,
                                                           const float* __restrict__ c1, const float* __restrict__ c2,
                                                           const float* __restrict__ c3, int C, int HW,
                                                           float* __restrict__ out_amax) {
  constexpr int UNR = 5;
  const int nblk = C >> 4;
  const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
  const int c = blk * 16 + (threadIdx.x & 3) * 4;
  const size_t gbase = (((size_t)b * (g_ctot >> 4) + ((g_coff >> 4) + blk)) * HW) * 16;
  const size_t zbase = (((size_t)b * (z_ctot >> 4) + ((z_coff >> 4) + blk)) * HW) * 16;
  const f32x4 k1 = *(const f32x4*)(c1 + c), k2 = *(const f32x4*)(c2 + c), k3 = *(const f32x4*)(c3 + c);
  const int n4 = HW * 4;
  float amax = 0.f;
  for (int i0 = threadIdx.x; i0 < n4; i0 += 256 * UNR) {
    f32x4 gv[UNR], zv[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int i = i0 + u * 256;
      const size_t o = (size_t)(i < n4 ? i : i0) * 4;       // (tail: re-read the first item, not stored)
      gv[u] = tsr_ld4<B16>(g, gbase + o);
      zv[u] = tsr_ld4<B16>(z, zbase + o);
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int i = i0 + u * 256;
      if (i < n4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          gv[u][j] = fmaf(k1[j], gv[u][j], fmaf(k2[j], zv[u][j], k3[j]));
          amax = fmaxf(amax, fabsf(gv[u][j]));
        }
        tsr_st4<B16>(g, gbase + (size_t)i * 4, gv[u]);
      }
    }
  }
  if (out_amax) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    if ((threadIdx.x & 63) == 0) publish_amax(out_amax, amax);
  }
}

extern "C" int tsr_bn_bwd_apply(float* g, int g_ctot, int g_coff, const float* z, int z_ctot, int z_coff,
                                const float* c1, const float* c2, const float* c3, int C, int B, int HW,
                                float* out_amax, void* stream) {
  if (!g || !z || !c1 || !c2 || !c3 || (C & 15) || (g_ctot & 15) || (g_coff & 15) || (z_ctot & 15) || (z_coff & 15) ||
      g_coff + C > g_ctot || z_coff + C > z_ctot)
    return TSR_ERR_ARG;
  if (B <= 0 || HW <= 0 || (long long)B * (C >> 4) > 0x7fffffffLL) return TSR_ERR_ARG;
  hipLaunchKernelGGL(bn_bwd_apply_kernel<false>, dim3(B * (C >> 4)), dim3(256), 0, (hipStream_t)stream,
                     g, g_ctot, g_coff, z, z_ctot, z_coff, c1, c2, c3, C, HW, out_amax);
  return tsr_check_launch();
}

// the same on bf16 CB16 tensors (training with bf16 activation storage): fp32 arithmetic, bf16 load / store
extern "C" int tsr_bn_bwd_apply_b16(void* g, int g_ctot, int g_coff, const void* z, int z_ctot, int z_coff,
                                    const float* c1, const float* c2, const float* c3, int C, int B, int HW,
                                    void* stream) {
  if (!g || !z || !c1 || !c2 || !c3 || (C & 15) || (g_ctot & 15) || (g_coff & 15) || (z_ctot & 15) || (z_coff & 15) ||
      g_coff + C > g_ctot || z_coff + C > z_ctot)
    return TSR_ERR_ARG;
  if (B <= 0 || HW <= 0 || (long long)B * (C >> 4) > 0x7fffffffLL) return TSR_ERR_ARG;
  hipLaunchKernelGGL(bn_bwd_apply_kernel<true>, dim3(B * (C >> 4)), dim3(256), 0, (hipStream_t)stream,
                     (float*)g, g_ctot, g_coff, (const float*)z, z_ctot, z_coff, c1, c2, c3, C, HW, (float*)nullptr);
  return tsr_check_launch();
}

// ------------------------------------------------------------------------------------------
// A BatchNorm2d layer in EVAL mode inside a training module (nn.BatchNorm2d.eval() under model.train(): it normalises with
// its running statistics and leaves them alone).  Forward: the same four per-channel vectors tsr_bn_stats_finalize hands
// out, from the running statistics; nothing is updated.  z is the bias-free accumulator, so the conv bias enters here.
// Backward: dz = scale * g (no batch-statistics terms), dgamma = sum g*xhat, dbeta = sum g.
// ------------------------------------------------------------------------------------------
__global__ void bn_eval_vectors_kernel(const float* __restrict__ bias, const float* __restrict__ gamma,
                                       const float* __restrict__ beta, const float* __restrict__ running_mean,
                                       const float* __restrict__ running_var, float eps, int C,
                                       float* __restrict__ scale, float* __restrict__ shift, float* __restrict__ xa,
                                       float* __restrict__ xb) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const double invstd = 1.0 / sqrt((double)running_var[c] + (double)eps);
  const double d = (bias ? (double)bias[c] : 0.0) - (double)running_mean[c];
  const double sc = (double)gamma[c] * invstd;
  scale[c] = (float)sc;
  shift[c] = (float)((double)beta[c] + d * sc);
  xa[c] = (float)invstd;
  xb[c] = (float)(d * invstd);
}

extern "C" int tsr_bn_eval_vectors(const float* bias, const float* gamma, const float* beta, const float* running_mean,
                                   const float* running_var, float eps, int C, float* scale, float* shift,
                                   float* xhat_a, float* xhat_b, void* stream) {
  if (!gamma || !beta || !running_mean || !running_var || !scale || !shift || !xhat_a || !xhat_b || C <= 0 || (C & 15))
    return TSR_ERR_ARG;
  hipLaunchKernelGGL(bn_eval_vectors_kernel, dim3((C + 63) / 64), dim3(64), 0, (hipStream_t)stream, bias, gamma, beta,
                     running_mean, running_var, eps, C, scale, shift, xhat_a, xhat_b);
  return tsr_check_launch();
}

// the tail of bn_bwd_final_kernel without the coefficients: part[k][c] = {entries, sum g, sum g*xhat}
__global__ void bn_bwd_final_eval_kernel(const double* __restrict__ part, int nblocks, int C, float* __restrict__ dgamma,
                                         float* __restrict__ dbeta) {
  __shared__ double sh[256 * 2];
  const int tid = threadIdx.x, cl = tid & 15, kl = tid >> 4;
  const int c = blockIdx.x * 16 + cl;
  double s1 = 0, s2 = 0;
  for (int k = kl; k < nblocks; k += 16) {
    const double* p = part + ((size_t)k * C + c) * 3;
    s1 += p[1]; s2 += p[2];
  }
  sh[tid * 2 + 0] = s1; sh[tid * 2 + 1] = s2;
  __syncthreads();
  if (kl != 0) return;
  for (int k = 1; k < 16; ++k) { s1 += sh[(k * 16 + cl) * 2 + 0]; s2 += sh[(k * 16 + cl) * 2 + 1]; }
  dbeta[c] = (float)s1;
  dgamma[c] = (float)s2;
}

extern "C" int tsr_bn_bwd_finalize_eval(const float* slab, int entries, int C, float* dgamma, float* dbeta, double* work,
                                        void* stream) {
  if (!slab || !dgamma || !dbeta || !work || entries <= 0 || (C != 64 && C != 128)) return TSR_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(slab_reduce_kernel, dim3(RED_BLOCKS), dim3(256), 0, st, slab, (const float*)nullptr, entries,
                     C, 1, work);
  hipLaunchKernelGGL(bn_bwd_final_eval_kernel, dim3(C / 16), dim3(256), 0, st, work, RED_BLOCKS, C, dgamma, dbeta);
  return tsr_check_launch();
}

// g[:, gcoff:gcoff+C] *= scale   (CB16, in place): one read and one write per element, no z.  The layout of
// bn_bwd_apply_kernel: one workgroup per (image, 16-channel block), a thread keeps one channel quad of `scale` and has UNR
// independent 16-B loads in flight.
template <bool B16>
__global__ __launch_bounds__(256) void bn_bwd_apply_eval_kernel(float* __restrict__ g, int g_ctot, int g_coff,
                                                                const float* __restrict__ scale, int C, int HW,
                                                                float* __restrict__ out_amax) {
  constexpr int UNR = 5;
  const int nblk = C >> 4;
  const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
  const int c = blk * 16 + (threadIdx.x & 3) * 4;
  const size_t gbase = (((size_t)b * (g_ctot >> 4) + ((g_coff >> 4) + blk)) * HW) * 16;
  const f32x4 k1 = *(const f32x4*)(scale + c);
  const int n4 = HW * 4;
  float amax = 0.f;
  for (int i0 = threadIdx.x; i0 < n4; i0 += 256 * UNR) {
    f32x4 gv[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int i = i0 + u * 256;
      gv[u] = tsr_ld4<B16>(g, gbase + (size_t)(i < n4 ? i : i0) * 4);       // (tail: re-read the first item, not stored)
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int i = i0 + u * 256;
      if (i < n4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          gv[u][j] *= k1[j];
          amax = fmaxf(amax, fabsf(gv[u][j]));
        }
        tsr_st4<B16>(g, gbase + (size_t)i * 4, gv[u]);
      }
    }
  }
  if (out_amax) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    if ((threadIdx.x & 63) == 0) publish_amax(out_amax, amax);
  }
}

static int bn_apply_eval_args(const void* g, int g_ctot, int g_coff, const float* scale, int C, int B, int HW) {
  if (!g || !scale || C <= 0 || (C & 15) || g_ctot <= 0 || (g_ctot & 15) || g_coff < 0 || (g_coff & 15) ||
      (long long)g_coff + C > g_ctot)
    return TSR_ERR_ARG;
  if (B <= 0 || HW <= 0 || HW > 0x7fffffff / 4 || (long long)B * (C >> 4) > 0x7fffffffLL) return TSR_ERR_ARG;
  return TSR_OK;
}

extern "C" int tsr_bn_bwd_apply_eval(float* g, int g_ctot, int g_coff, const float* scale, int C, int B, int HW,
                                     float* out_amax, void* stream) {
  if (bn_apply_eval_args(g, g_ctot, g_coff, scale, C, B, HW)) return TSR_ERR_ARG;
  hipLaunchKernelGGL(bn_bwd_apply_eval_kernel<false>, dim3(B * (C >> 4)), dim3(256), 0, (hipStream_t)stream, g, g_ctot,
                     g_coff, scale, C, HW, out_amax);
  return tsr_check_launch();
}

// the same on a bf16 CB16 tensor: fp32 product, rounded once on the store
extern "C" int tsr_bn_bwd_apply_eval_b16(void* g, int g_ctot, int g_coff, const float* scale, int C, int B, int HW,
                                         void* stream) {
  if (bn_apply_eval_args(g, g_ctot, g_coff, scale, C, B, HW)) return TSR_ERR_ARG;
  hipLaunchKernelGGL(bn_bwd_apply_eval_kernel<true>, dim3(B * (C >> 4)), dim3(256), 0, (hipStream_t)stream, (float*)g,
                     g_ctot, g_coff, scale, C, HW, (float*)nullptr);
  return tsr_check_launch();
}

// ------------------------------------------------------------------------------------------
// stem backward: dW[64][3][3][3] of Upsample+Conv2d(3->64) (the taxel gradient: stem_dgrad_kernel below)
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void bilin_src_t(int dst, float scale, int n_in, int& i0, int& i1, float& lam) {
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  i0 = (int)src;
  i0 = i0 < n_in - 1 ? i0 : n_in - 1;
  i1 = i0 + 1 < n_in ? i0 + 1 : n_in - 1;
  lam = src - (float)i0;
}

// one workgroup per (image split, band group); thread = (co = tid&63, pixel phase = tid>>6).  `bands` > 1 for tall images:
// a workgroup then holds only one band of the upsampled image (+ one halo row each side) in LDS at a time -- at 100 x 100 the
// whole image is 125 KB, i.e. one workgroup per CU.  The slab entries are (band group, image split) pairs, nsplit in all:
// gridDim.y band groups (a divisor of nsplit), a workgroup walks the bands blockIdx.y, blockIdx.y + gridDim.y, .. of its images.
template <bool B16>
__global__ __launch_bounds__(256) void stem_wgrad_kernel(const float* __restrict__ lr, int lr_ctot, int lr_coff,
                                                         int hin, int win, int sf, const float* __restrict__ dz,
                                                         int dz_ctot, int dz_coff, float* __restrict__ slab, int B,
                                                         int bands) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int Himg = hin * sf, W = win * sf, WP = W + 2;
  const int RBAND = (Himg + bands - 1) / bands;
  const int HP = RBAND + 2;
  float* tax = smem;                                   // [3][hin*win]
  float* up = smem + ((3 * hin * win + 3) & ~3);       // [3][HP][WP] zero padded: band rows yb0 - 1 .. yb0 + RBAND
  const int tid = threadIdx.x;
  const int co = tid & 63, ph = tid >> 6;
  const int HW = Himg * W;
  float acc[27];
#pragma unroll
  for (int k = 0; k < 27; ++k) acc[k] = 0.f;
  const float sc = 1.0f / (float)sf;
  const int oc = dz_coff + co;
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    __syncthreads();
    for (int i = tid; i < 3 * hin * win; i += 256) tax[i] = lr[((size_t)b * lr_ctot + lr_coff) * hin * win + i];
    for (int bd = blockIdx.y; bd < bands; bd += gridDim.y) {
      const int yb0 = bd * RBAND;
      const int H = Himg - yb0 < RBAND ? Himg - yb0 : RBAND;      // rows of this band
      __syncthreads();
      for (int i = tid; i < 3 * HP * WP; i += 256) {
        const int c = i / (HP * WP), rem = i - c * (HP * WP);
        const int gy = yb0 + rem / WP - 1, gx = rem % WP - 1;
        float v = 0.f;
        if (gy >= 0 && gy < Himg && gx >= 0 && gx < W) {
          int ya, yb, xa, xb; float ly, lx;
          bilin_src_t(gy, sc, hin, ya, yb, ly);
          bilin_src_t(gx, sc, win, xa, xb, lx);
          const float* t = tax + c * hin * win;
          const float top = (1.f - lx) * t[ya * win + xa] + lx * t[ya * win + xb];
          const float bot = (1.f - lx) * t[yb * win + xa] + lx * t[yb * win + xb];
          v = (1.f - ly) * top + ly * bot;
        }
        up[i] = v;
      }
      __syncthreads();
      const size_t dzo = (((size_t)b * (dz_ctot >> 4) + (oc >> 4)) * HW) * 16 + (oc & 15);
      // A wave walks whole rows (y = ph, ph + 4, ..) in chunks of PU pixels.  The PU gradient loads of a chunk are requested
      // together (one dependent 2- / 4-byte load per pixel made the loop a chain of memory latencies: 0.78 ms per launch at
      // B = 2048 for 0.42 GB), and the 3x3x3 window of the upsampled image slides in registers: column x + 3 replaces column x
      // (9 LDS reads per pixel instead of 27; the reads are broadcasts -- all 64 lanes of a wave share the pixel).
      constexpr int PU = 8;
      for (int y = ph; y < H; y += 4) {
        for (int x0 = 0; x0 < W; x0 += PU) {
          float d[PU];
#pragma unroll
          for (int u = 0; u < PU; ++u) {
            const int x = x0 + u;
            const float v = tsr_ld1<B16>(dz, dzo + (size_t)((yb0 + y) * W + (x < W ? x : x0)) * 16);
            d[u] = x < W ? v : 0.f;                  // (a chunk's tail beyond the row adds nothing; its window reads stay in the padding)
          }
          float col[3][9];                           // col[(x - x0) % 3][c * 3 + kh] = up[c][y + kh][x]
#pragma unroll
          for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int r = 0; r < 9; ++r) col[j][r] = up[((r / 3) * HP + y + (r % 3)) * WP + x0 + j];
#pragma unroll
          for (int u = 0; u < PU; ++u) {
#pragma unroll
            for (int r = 0; r < 9; ++r)
#pragma unroll
              for (int kw = 0; kw < 3; ++kw) acc[r * 3 + kw] = fmaf(d[u], col[(u + kw) % 3][r], acc[r * 3 + kw]);
            if (u + 1 < PU) {
              const int xn = x0 + u + 3 < WP ? x0 + u + 3 : WP - 1;          // (past the padded row only under a zero gradient)
#pragma unroll
              for (int r = 0; r < 9; ++r) col[u % 3][r] = up[((r / 3) * HP + y + (r % 3)) * WP + xn];
            }
          }
        }
      }
    }
  }
  // combine the 4 pixel phases through LDS, write this split's OIHW partial
  __syncthreads();
  float* red = smem;   // reuse: [4][64][27]
#pragma unroll
  for (int k = 0; k < 27; ++k) red[(ph * 64 + co) * 27 + k] = acc[k];
  __syncthreads();
  for (int i = tid; i < 64 * 27; i += 256)
    slab[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 64 * 27 + i] =
        (red[i] + red[64 * 27 + i]) + (red[2 * 64 * 27 + i] + red[3 * 64 * 27 + i]);
}

static int stem_wgrad_impl(const float* lr, int lr_ctot, int lr_coff, int hin, int win, int sf,
                           const float* dz, int dz_ctot, int dz_coff, float* slab, int nsplit, int B,
                           void* stream, bool b16) {
  if (!lr || !dz || !slab || nsplit <= 0 || B <= 0 || (dz_ctot & 15) || (dz_coff & 15) || dz_coff + 64 > dz_ctot)
    return TSR_ERR_ARG;
  const int H = hin * sf, W = win * sf;
  if (hin <= 0 || win <= 0 || sf <= 0) return TSR_ERR_ARG;
  // LDS floats of a workgroup that holds `bands` bands of rows per image (one at a time, + halo rows)
  auto lds_floats = [&](int bands) {
    const size_t fl = ((3 * hin * win + 3) & ~3) + (size_t)3 * ((H + bands - 1) / bands + 2) * (W + 2);
    return fl < 4 * 64 * 27 ? (size_t)4 * 64 * 27 : fl;
  };
  // band groups across the grid: the band (+ halo) within 32 KB of LDS, as far as they divide the splits (slab entries =
  // nsplit either way); then bands per image, a multiple of the groups, until the band fits the 160 KB LDS at all
  int groups = 1;
  while (groups < 8 && lds_floats(groups) * 4 > 32 * 1024 && nsplit % (2 * groups) == 0) groups *= 2;
  int bands = groups;
  while (bands < H && lds_floats(bands) * 4 > 160 * 1024) bands *= 2;
  const size_t fl = lds_floats(bands);
  if (fl * 4 > 160 * 1024) return TSR_ERR_ARG;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)stem_wgrad_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void*)stem_wgrad_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr_set = true;
  }
  if (b16)
    hipLaunchKernelGGL(stem_wgrad_kernel<true>, dim3(nsplit / groups, groups), dim3(256), fl * 4, (hipStream_t)stream, lr, lr_ctot,
                       lr_coff, hin, win, sf, dz, dz_ctot, dz_coff, slab, B, bands);
  else
    hipLaunchKernelGGL(stem_wgrad_kernel<false>, dim3(nsplit / groups, groups), dim3(256), fl * 4, (hipStream_t)stream, lr, lr_ctot,
                       lr_coff, hin, win, sf, dz, dz_ctot, dz_coff, slab, B, bands);
  return tsr_check_launch();
}

extern "C" int tsr_stem_wgrad(const float* lr, int lr_ctot, int lr_coff, int hin, int win, int sf,
                              const float* dz, int dz_ctot, int dz_coff, float* slab, int nsplit, int B,
                              void* stream) {
  return stem_wgrad_impl(lr, lr_ctot, lr_coff, hin, win, sf, dz, dz_ctot, dz_coff, slab, nsplit, B, stream, false);
}

// dz is a bf16 CB16 tensor (training with bf16 activation storage)
extern "C" int tsr_stem_wgrad_b16(const float* lr, int lr_ctot, int lr_coff, int hin, int win, int sf,
                                  const void* dz, int dz_ctot, int dz_coff, float* slab, int nsplit, int B,
                                  void* stream) {
  return stem_wgrad_impl(lr, lr_ctot, lr_coff, hin, win, sf, (const float*)dz, dz_ctot, dz_coff, slab, nsplit, B, stream, true);
}

// ------------------------------------------------------------------------------------------
// stem data gradient: dx[3][hin][win] of z = conv3x3(up_sf(x), W) given dz (reference model/tactileSR_model.py:35-37,60-61)
//   t[c][kh][kw](p) = sum_co W[co][c][kh][kw] dz[co][p]      -- dz pixel p feeds dup at q = p + (kh - 1, kw - 1)
//   dx[c][i][j]    += A_y[q_y][i] A_x[q_x][j] t[c][kh][kw](p) for q inside the image (the conv's zero padding drops the rest)
// One workgroup per image owns its 3 x hin x win outputs: no float atomics, the same bits on every run.  A thread walks the
// pixels p = tid, tid + 256, ..; it reads each dz pixel once (64 channels = four 64-B CB16 lines, as 16-B loads), the
// 27 x 64 weights are wave-uniform loads (scalar cache), and the bilinear adjoint is two small contractions against per-row /
// per-column tap tables in LDS: tab[r][k][i] = weight of taxel i in upsampled row r + k - 1 (0 outside the image; clamped
// edge taps add up).  Per-thread partials meet through a fixed shuffle tree and a fixed-order sum over the 4 waves.
// ------------------------------------------------------------------------------------------
#define STEM_DG_MAXT 4     // taxels per axis (TactileSR: 4 x 4)

template <bool B16>
__global__ __launch_bounds__(256) void stem_dgrad_kernel(const float* __restrict__ w, const float* __restrict__ dz,
                                                         int dz_ctot, int dz_coff, int hin, int win, int sf,
                                                         float* __restrict__ dx, int dx_ctot, int dx_coff, int accumulate) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int H = hin * sf, W = win * sf, HW = H * W;
  float* taby = smem;                                  // [H][3][4]
  float* tabx = smem + H * 12;                         // [W][3][4]
  float* red = tabx + W * 12;                          // [4 waves][48]
  const int tid = threadIdx.x, b = blockIdx.x;
  const float sc = 1.0f / (float)sf;
  for (int e = tid; e < (H + W) * 3; e += 256) {
    const bool isy = e < H * 3;
    const int k = isy ? e : e - H * 3;
    const int r = k / 3, kk = k - r * 3, n = isy ? H : W, nin = isy ? hin : win;
    const int q = r + kk - 1;
    float v[STEM_DG_MAXT] = {0.f, 0.f, 0.f, 0.f};
    if (q >= 0 && q < n) {
      int i0, i1; float lam;
      bilin_src_t(q, sc, nin, i0, i1, lam);
#pragma unroll
      for (int i = 0; i < STEM_DG_MAXT; ++i) v[i] = (i == i0 ? 1.f - lam : 0.f) + (i == i1 ? lam : 0.f);
    }
    *(f32x4*)((isy ? taby : tabx) + k * 4) = (f32x4){v[0], v[1], v[2], v[3]};
  }
  __syncthreads();
  float acc[3][STEM_DG_MAXT][STEM_DG_MAXT];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int i = 0; i < STEM_DG_MAXT; ++i)
#pragma unroll
      for (int j = 0; j < STEM_DG_MAXT; ++j) acc[c][i][j] = 0.f;
  const size_t plane = (size_t)HW * 16;
  const size_t base = ((size_t)b * (dz_ctot >> 4) + (dz_coff >> 4)) * plane;
  for (int p = tid; p < HW; p += 256) {
    float d[64];
#pragma unroll
    for (int blk = 0; blk < 4; ++blk)
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const f32x4 v = tsr_ld4<B16>(dz, base + blk * plane + (size_t)p * 16 + q4 * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) d[blk * 16 + q4 * 4 + e] = v[e];
      }
    float t[27];
#pragma unroll
    for (int r = 0; r < 27; ++r) t[r] = 0.f;
#pragma unroll
    for (int co = 0; co < 64; co += 2) {
      // the weights come through the scalar cache, two rows per step: the empty asm keeps the compiler from hoisting all
      // 1728 uniform loads out of the pixel loop (they would not fit in SGPRs and spill)
      int wo = co * 27;
      asm volatile("" : "+s"(wo));
      const float* wr = w + wo;
#pragma unroll
      for (int r = 0; r < 27; ++r) t[r] = fmaf(wr[27 + r], d[co + 1], fmaf(wr[r], d[co], t[r]));
    }
    const int y = p / W, x = p - y * W;
    f32x4 ty[3], tx[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      ty[k] = *(const f32x4*)(taby + (y * 3 + k) * 4);
      tx[k] = *(const f32x4*)(tabx + (x * 3 + k) * 4);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        float u[STEM_DG_MAXT];                         // u[j] = sum_kw A_x(x + kw - 1, j) t[c][kh][kw]
#pragma unroll
        for (int j = 0; j < STEM_DG_MAXT; ++j)
          u[j] = fmaf(tx[2][j], t[c * 9 + kh * 3 + 2], fmaf(tx[1][j], t[c * 9 + kh * 3 + 1], tx[0][j] * t[c * 9 + kh * 3]));
#pragma unroll
        for (int i = 0; i < STEM_DG_MAXT; ++i)
#pragma unroll
          for (int j = 0; j < STEM_DG_MAXT; ++j) acc[c][i][j] = fmaf(ty[kh][i], u[j], acc[c][i][j]);
      }
  }
  // fixed-order reduction: butterfly within the wave, then the 4 wave partials in wave order
  const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int i = 0; i < STEM_DG_MAXT; ++i)
#pragma unroll
      for (int j = 0; j < STEM_DG_MAXT; ++j) {
        float v = acc[c][i][j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) red[wv * 48 + (c * STEM_DG_MAXT + i) * STEM_DG_MAXT + j] = v;
      }
  __syncthreads();
  if (tid < 48) {
    const int c = tid / 16, i = (tid >> 2) & 3, j = tid & 3;
    if (i < hin && j < win) {
      const float v = (red[tid] + red[48 + tid]) + (red[96 + tid] + red[144 + tid]);
      float* o = dx + (((size_t)b * dx_ctot + dx_coff + c) * hin + i) * win + j;
      *o = accumulate ? *o + v : v;
    }
  }
}

static int stem_dgrad_impl(const float* w_oihw, const float* dz, int dz_ctot, int dz_coff, int hin, int win, int sf,
                           float* dx, int dx_ctot, int dx_coff, int accumulate, int B, void* stream, bool b16) {
  if (!w_oihw || !dz || !dx || B <= 0 || hin <= 0 || win <= 0 || sf <= 0 || hin > STEM_DG_MAXT || win > STEM_DG_MAXT ||
      (dz_ctot & 15) || (dz_coff & 15) || dz_coff < 0 || dz_coff + 64 > dz_ctot || dx_coff < 0 || dx_coff + 3 > dx_ctot ||
      (accumulate != 0 && accumulate != 1))
    return TSR_ERR_ARG;
  const size_t fl = (size_t)(hin + win) * sf * 12 + 4 * 48;
  if (fl * 4 > 64 * 1024) return TSR_ERR_ARG;
  if (b16)
    hipLaunchKernelGGL(stem_dgrad_kernel<true>, dim3(B), dim3(256), fl * 4, (hipStream_t)stream, w_oihw, dz, dz_ctot,
                       dz_coff, hin, win, sf, dx, dx_ctot, dx_coff, accumulate);
  else
    hipLaunchKernelGGL(stem_dgrad_kernel<false>, dim3(B), dim3(256), fl * 4, (hipStream_t)stream, w_oihw, dz, dz_ctot,
                       dz_coff, hin, win, sf, dx, dx_ctot, dx_coff, accumulate);
  return tsr_check_launch();
}

extern "C" int tsr_stem_dgrad(const float* w_oihw, const float* dz, int dz_ctot, int dz_coff, int hin, int win, int sf,
                              float* dx, int dx_ctot, int dx_coff, int accumulate, int B, void* stream) {
  return stem_dgrad_impl(w_oihw, dz, dz_ctot, dz_coff, hin, win, sf, dx, dx_ctot, dx_coff, accumulate, B, stream, false);
}

// dz is a bf16 CB16 tensor (training with bf16 activation storage); fp32 arithmetic
extern "C" int tsr_stem_dgrad_b16(const float* w_oihw, const void* dz, int dz_ctot, int dz_coff, int hin, int win, int sf,
                                  float* dx, int dx_ctot, int dx_coff, int accumulate, int B, void* stream) {
  return stem_dgrad_impl(w_oihw, (const float*)dz, dz_ctot, dz_coff, hin, win, sf, dx, dx_ctot, dx_coff, accumulate, B,
                         stream, true);
}

// ------------------------------------------------------------------------------------------
// head backward.  out = relu(conv3x3(h0; w[1][C][3][3])), dout given NCHW (B,1,H,W).
//   dpre = dout*[out>0];  dh0[c,q] = sum_tap dpre[q - tap + 1]*w[c][tap];  dz_h0 = dh0*[h0>0]
//   dW[c][tap] = sum_{b,q} dpre[q - tap + 1]*h0[c][q]  (flipped correlation: out pixel p = q - (tap-1))
// ------------------------------------------------------------------------------------------
template <bool B16>
__global__ __launch_bounds__(256) void head_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ out,
                                                       const float* __restrict__ h0, int h_ctot, int cin,
                                                       const float* __restrict__ w, float* __restrict__ dz,
                                                       int dz_ctot, int B, int H, int W, float* __restrict__ out_amax) {
  extern __shared__ __attribute__((aligned(16))) float wl[];   // [9][cin]
  const int tid = threadIdx.x;
  for (int i = tid; i < 9 * cin; i += 256) {
    const int c = i % cin, tap = i / cin;
    wl[i] = w[c * 9 + tap];
  }
  __syncthreads();
  const int HW = H * W, b = blockIdx.y, nblk = cin >> 4;
  // item = (pixel, channel quad), looping over the channel blocks: the nine masked dout neighbours of the pixel are
  // gathered ONCE per thread and reused for every block (round 2 made the block part of the item: each of the 32 threads
  // of a pixel repeated the 18 small loads -- 3.4 ms per step at B = 2048, 1 TB/s on a kernel that moves 3.4 GB).  The
  // four lanes of a quad still cover one 64-B CB16 line, a wave 16 whole lines per load / store instruction.
  const int item = blockIdx.x * 256 + tid;
  float amax = 0.f;
  if (item < HW * 4) {
    const int qd = item & 3, q = item >> 2;
    const int y = q / W, x = q - y * W;
    float dp[9];
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int py = y - kh + 1, px = x - kw + 1;
        float v = 0.f;
        if (py >= 0 && py < H && px >= 0 && px < W) {
          const size_t o = (size_t)b * HW + py * W + px;
          v = out[o] > 0.f ? dout[o] : 0.f;
        }
        dp[kh * 3 + kw] = v;
      }
    for (int blk = 0; blk < nblk; ++blk) {
      const size_t eo = (((size_t)b * (h_ctot >> 4) + blk) * HW + q) * 16 + qd * 4;
      const size_t zo = (((size_t)b * (dz_ctot >> 4) + blk) * HW + q) * 16 + qd * 4;
      const f32x4 hv = tsr_ld4<B16>(h0, eo);
      f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const f32x4 wv = *(const f32x4*)(wl + t * cin + blk * 16 + qd * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) s4[j] = fmaf(dp[t], wv[j], s4[j]);
      }
      f32x4 r;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        r[j] = hv[j] > 0.f ? s4[j] : 0.f;
        amax = fmaxf(amax, fabsf(r[j]));
      }
      tsr_st4<B16>(dz, zo, r);
    }
  }
  if (out_amax) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    if ((tid & 63) == 0) publish_amax(out_amax, amax);
  }
}

// thread = channel c (cin <= 256 => one thread per channel, remaining threads idle), grid = splits
template <bool B16>
__global__ __launch_bounds__(256) void head_wgrad_kernel(const float* __restrict__ dout, const float* __restrict__ out,
                                                         const float* __restrict__ h0, int h_ctot, int cin,
                                                         float* __restrict__ slab, int B, int H, int W, int nsplit) {
  extern __shared__ __attribute__((aligned(16))) float dpt[];   // [(H+2)*(W+2)] masked dout, zero padded
  const int tid = threadIdx.x;
  const int HW = H * W, WP = W + 2;
  const int ngrp = 256 / cin;                     // pixel phases
  const int c = tid % cin, ph = tid / cin;
  float acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = 0.f;
  for (int b = blockIdx.x; b < B; b += nsplit) {
    __syncthreads();
    for (int i = tid; i < (H + 2) * WP; i += 256) {
      const int py = i / WP - 1, px = i % WP - 1;
      float v = 0.f;
      if (py >= 0 && py < H && px >= 0 && px < W) {
        const size_t o = (size_t)b * HW + py * W + px;
        v = out[o] > 0.f ? dout[o] : 0.f;
      }
      dpt[i] = v;
    }
    __syncthreads();
    if (ph < ngrp) {
      const size_t ho = (((size_t)b * (h_ctot >> 4) + (c >> 4)) * HW) * 16 + (c & 15);
      // rows y = ph, ph + ngrp, .. in chunks of PU pixels: the chunk's activation loads are requested together (one dependent
      // 2- / 4-byte load per pixel was a chain of memory latencies) and the 3x3 window of the masked output gradient slides in
      // registers (out pixel p = q - (tap - 1); padded index + 1: tap (kh, kw) of pixel x reads column x - kw + 2)
      constexpr int PU = 8;
      for (int y = ph; y < H; y += ngrp) {
        for (int x0 = 0; x0 < W; x0 += PU) {
          float hv[PU];
#pragma unroll
          for (int u = 0; u < PU; ++u) {
            const int x = x0 + u;
            const float v = tsr_ld1<B16>(h0, ho + (size_t)(y * W + (x < W ? x : x0)) * 16);
            hv[u] = x < W ? v : 0.f;
          }
          float col[3][3];                     // col[j % 3][kh] = dpt[y - kh + 2][x0 + j]
#pragma unroll
          for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) col[j][kh] = dpt[(y - kh + 2) * WP + x0 + j];
#pragma unroll
          for (int u = 0; u < PU; ++u) {
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
              for (int kw = 0; kw < 3; ++kw) acc[kh * 3 + kw] = fmaf(hv[u], col[(u + 2 - kw) % 3][kh], acc[kh * 3 + kw]);
            if (u + 1 < PU) {
              const int xn = x0 + u + 3 < WP ? x0 + u + 3 : WP - 1;
#pragma unroll
              for (int kh = 0; kh < 3; ++kh) col[u % 3][kh] = dpt[(y - kh + 2) * WP + xn];
            }
          }
        }
      }
    }
  }
  __syncthreads();
  float* red = dpt;     // [ngrp][cin][9]
  if (ph < ngrp)
#pragma unroll
    for (int t = 0; t < 9; ++t) red[(ph * cin + c) * 9 + t] = acc[t];
  __syncthreads();
  for (int i = tid; i < cin * 9; i += 256) {
    float s = 0.f;
    for (int k = 0; k < ngrp; ++k) s += red[k * cin * 9 + i];
    slab[(size_t)blockIdx.x * cin * 9 + i] = s;
  }
}

template <bool B16>
static int head_bwd_impl(const float* dout, const float* out, const float* h0, int h_ctot, int cin,
                         const float* w_oihw, float* dz_h0, int dz_ctot, float* wslab, int nsplit,
                         int B, int H, int W, float* dz_amax, void* stream) {
  if (!dout || !out || !h0 || !w_oihw || !dz_h0 || !wslab || nsplit <= 0 || (cin & 15) || cin > 256 || cin > h_ctot ||
      cin > dz_ctot || (h_ctot & 15) || (dz_ctot & 15) || B <= 0 || H <= 0 || W <= 0)
    return TSR_ERR_ARG;
  // head_wgrad_kernel keeps the whole zero-padded masked dout image in LDS: (H + 2)(W + 2) floats within 64 KB, i.e. at most
  // 126 x 126 (4 x 4 taxels: scale_factor <= 31).  Checked before the first launch: a refused call writes nothing.
  size_t fl = (size_t)(H + 2) * (W + 2);
  const size_t redf = (size_t)(256 / cin) * cin * 9;
  if (fl < redf) fl = redf;
  if (fl * 4 > 64 * 1024) return TSR_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int items = H * W * 4;
  hipLaunchKernelGGL(head_bwd_kernel<B16>, dim3((items + 255) / 256, B), dim3(256), (size_t)9 * cin * 4, st, dout, out,
                     h0, h_ctot, cin, w_oihw, dz_h0, dz_ctot, B, H, W, dz_amax);
  hipLaunchKernelGGL(head_wgrad_kernel<B16>, dim3(nsplit), dim3(256), fl * 4, st, dout, out, h0, h_ctot, cin, wslab, B, H,
                     W, nsplit);
  return tsr_check_launch();
}

extern "C" int tsr_head_bwd(const float* dout, const float* out, const float* h0, int h_ctot, int cin,
                            const float* w_oihw, float* dz_h0, int dz_ctot, float* wslab, int nsplit,
                            int B, int H, int W, float* dz_amax, void* stream) {
  return head_bwd_impl<false>(dout, out, h0, h_ctot, cin, w_oihw, dz_h0, dz_ctot, wslab, nsplit, B, H, W, dz_amax, stream);
}

// h0 and dz_h0 are bf16 CB16 tensors (training with bf16 activation storage); dout / out stay fp32 NCHW
extern "C" int tsr_head_bwd_b16(const float* dout, const float* out, const void* h0, int h_ctot, int cin,
                                const float* w_oihw, void* dz_h0, int dz_ctot, float* wslab, int nsplit,
                                int B, int H, int W, void* stream) {
  return head_bwd_impl<true>(dout, out, (const float*)h0, h_ctot, cin, w_oihw, (float*)dz_h0, dz_ctot, wslab, nsplit, B, H,
                             W, nullptr, stream);
}

// The activation-gradient half of tsr_head_bwd alone (a frozen output_layer.2.weight whose dz_h0 is still consumed): the same
// head_bwd_kernel launch, so dz_h0 / dz_amax carry tsr_head_bwd's bits.  No LDS bound: that one is head_wgrad_kernel's.
template <bool B16>
static int head_dgrad_impl(const float* dout, const float* out, const float* h0, int h_ctot, int cin, const float* w_oihw,
                           float* dz_h0, int dz_ctot, int B, int H, int W, float* dz_amax, void* stream) {
  if (!dout || !out || !h0 || !w_oihw || !dz_h0 || (cin & 15) || cin > 256 || cin > h_ctot || cin > dz_ctot ||
      (h_ctot & 15) || (dz_ctot & 15) || B <= 0 || H <= 0 || W <= 0)
    return TSR_ERR_ARG;
  if ((long long)H * W > (1 << 28)) return TSR_ERR_ARG;      // the kernel's (pixel, channel quad) item index is an int
  const int items = H * W * 4;
  hipLaunchKernelGGL(head_bwd_kernel<B16>, dim3((items + 255) / 256, B), dim3(256), (size_t)9 * cin * 4, (hipStream_t)stream,
                     dout, out, h0, h_ctot, cin, w_oihw, dz_h0, dz_ctot, B, H, W, dz_amax);
  return tsr_check_launch();
}

extern "C" int tsr_head_dgrad(const float* dout, const float* out, const float* h0, int h_ctot, int cin,
                              const float* w_oihw, float* dz_h0, int dz_ctot, int B, int H, int W, float* dz_amax,
                              void* stream) {
  return head_dgrad_impl<false>(dout, out, h0, h_ctot, cin, w_oihw, dz_h0, dz_ctot, B, H, W, dz_amax, stream);
}

extern "C" int tsr_head_dgrad_b16(const float* dout, const float* out, const void* h0, int h_ctot, int cin,
                                  const float* w_oihw, void* dz_h0, int dz_ctot, int B, int H, int W, void* stream) {
  return head_dgrad_impl<true>(dout, out, (const float*)h0, h_ctot, cin, w_oihw, (float*)dz_h0, dz_ctot, B, H, W, nullptr,
                               stream);
}

// ------------------------------------------------------------------------------------------
// target preparation: HR_raw (B,1,hin,win) * inv_scale -> bilinear (align_corners=False) to (H,W)
// (train/tactileSR_train.py:44-45: HR/HR_scale_num, F.interpolate(size=(4sf,4sf)))
// ------------------------------------------------------------------------------------------
__global__ void target_prep_kernel(const float* __restrict__ hr, float* __restrict__ out, float inv_scale, int B,
                                   int hin, int win, int H, int W) {
  const size_t total = (size_t)B * H * W;
  const float sy = (float)hin / (float)H, sx = (float)win / (float)W;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int x = i % W; size_t r = i / W;
    const int y = r % H; const int b = r / H;
    int ya, yb, xa, xb; float ly, lx;
    bilin_src_t(y, sy, hin, ya, yb, ly);
    bilin_src_t(x, sx, win, xa, xb, lx);
    const float* t = hr + (size_t)b * hin * win;
    const float v00 = t[ya * win + xa] * inv_scale, v01 = t[ya * win + xb] * inv_scale;
    const float v10 = t[yb * win + xa] * inv_scale, v11 = t[yb * win + xb] * inv_scale;
    out[i] = (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
  }
}

extern "C" int tsr_target_prep(const float* hr_raw, float* out, float inv_scale, int B, int hin, int win, int H,
                               int W, void* stream) {
  if (!hr_raw || !out || B <= 0) return TSR_ERR_ARG;
  const size_t total = (size_t)B * H * W;
  const size_t g = (total + 255) / 256;
  hipLaunchKernelGGL(target_prep_kernel, dim3(g > 8192 ? 8192 : (int)g), dim3(256), 0, (hipStream_t)stream, hr_raw,
                     out, inv_scale, B, hin, win, H, W);
  return tsr_check_launch();
}

// ------------------------------------------------------------------------------------------
// MSE loss (mean over all elements) forward + backward in one pass:
//   partial[block] = sum (y-t)^2 (fp64), dy = gscale * 2 (y-t) / n ; loss = sum(partial)/n (second kernel)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mse_kernel(const float* __restrict__ y, const float* __restrict__ t,
                                                  float* __restrict__ dy, size_t n, float gcoef,
                                                  double* __restrict__ part) {
  __shared__ double sh[256];
  double s = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float d = y[i] - t[i];
    s += (double)d * (double)d;
    if (dy) dy[i] = gcoef * d;
  }
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (threadIdx.x < k) sh[threadIdx.x] += sh[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

__global__ void mse_final_kernel(const double* __restrict__ part, int nb, double inv_n, float* __restrict__ loss) {
  double s = 0;
  for (int k = 0; k < nb; ++k) s += part[k];
  loss[0] = (float)(s * inv_n);
}

extern "C" int tsr_mse_fwd_bwd(const float* y, const float* target, float* dy, float* loss, long long n,
                               float grad_scale, double* work, void* stream) {
  if (!y || !target || !loss || !work || n <= 0) return TSR_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int nb = 256;
  hipLaunchKernelGGL(mse_kernel, dim3(nb), dim3(256), 0, st, y, target, dy, (size_t)n,
                     (float)(2.0 * grad_scale / (double)n), work);
  hipLaunchKernelGGL(mse_final_kernel, dim3(1), dim3(1), 0, st, work, nb, 1.0 / (double)n, loss);
  return tsr_check_launch();
}

// ------------------------------------------------------------------------------------------
// Adam with L2-in-gradient weight decay (torch.optim.Adam, not AdamW), one tensor per launch.
//   g' = g + wd*p ; m = b1 m + (1-b1) g' ; v = b2 v + (1-b2) g'^2
//   p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
// ------------------------------------------------------------------------------------------
__global__ void adam_l2_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                               float* __restrict__ v, size_t n, float lr, float b1, float b2, float omb1, float omb2,
                               float eps, float wd, float bc1, float bc2_sqrt) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float w = p[i];
    const float gg = fmaf(wd, w, g[i]);
    const float mm = b1 * m[i] + omb1 * gg;
    const float vv = b2 * v[i] + omb2 * gg * gg;
    m[i] = mm;
    v[i] = vv;
    const float denom = sqrtf(vv) / bc2_sqrt + eps;
    p[i] = w - (lr / bc1) * (mm / denom);
  }
}

extern "C" int tsr_adam_l2_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n,
                                float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                                void* stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq || n <= 0 || step <= 0) return TSR_ERR_ARG;
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  const size_t g = ((size_t)n + 255) / 256;
  hipLaunchKernelGGL(adam_l2_kernel, dim3(g > 4096 ? 4096 : (int)g), dim3(256), 0, (hipStream_t)stream, param, grad,
                     exp_avg, exp_avg_sq, (size_t)n, lr, beta1, beta2, (float)(1.0 - (double)beta1),
                     (float)(1.0 - (double)beta2), eps, weight_decay, (float)bc1, (float)sqrt(bc2));
  return tsr_check_launch();
}

// One launch for all parameter tensors: block b owns chunk record b (<= 4096 contiguous elements of one tensor).
// 16-B accesses when the four pointers are 16-B aligned (torch allocations and the gradient arena are).
// The body is shared by the launch forms below: per-step scalars as kernel arguments (tsr_adam_l2_multi) or read
// from device memory (tsr_adam_l2_multi_dev, the graph-captured step), each with or without gradient clipping (CLIP:
// the gradient is first multiplied by the coefficient *clip that tsr_grad_norm_multi wrote, as its own rounded value,
// and written back -- torch's clip_grad_norm_ leaves p.grad clipped).  The CLIP = false forms are the plain step.
template <bool CLIP>
__device__ __forceinline__ void adam_l2_multi_body(const tsr_adam_chunk* __restrict__ chunks, float lr, float b1,
                                                   float b2, float omb1, float omb2, float eps, float wd, float bc1,
                                                   float bc2_sqrt, const float* __restrict__ clip) {
  const tsr_adam_chunk c = chunks[blockIdx.x];
  const float step_size = lr / bc1;
  auto upd = [&](float w, float g, float& m, float& v) {
    const float gg = fmaf(wd, w, g);
    m = b1 * m + omb1 * gg;
    v = b2 * v + omb2 * gg * gg;
    return w - step_size * (m / (sqrtf(v) / bc2_sqrt + eps));
  };
  float coef = 1.0f;
  if (CLIP) coef = clip[0];
  // coef == 1 multiplies exactly: the gradient already holds the clipped value (NaN != 1: a NaN coefficient writes)
  const bool write_grad = CLIP && !(coef == 1.0f);
  float* grad_out = const_cast<float*>(c.grad);
  const bool vec = ((((size_t)c.param | (size_t)c.grad | (size_t)c.exp_avg | (size_t)c.exp_avg_sq) & 15) == 0);
  const int n4 = vec ? (c.n >> 2) : 0;
  for (int i = threadIdx.x; i < n4; i += 256) {
    f32x4 w = ((f32x4*)c.param)[i], m = ((f32x4*)c.exp_avg)[i], v = ((f32x4*)c.exp_avg_sq)[i];
    f32x4 g = ((const f32x4*)c.grad)[i];
    if (CLIP) {
#pragma unroll
      for (int j = 0; j < 4; ++j) g[j] = __fmul_rn(g[j], coef);
      if (write_grad) ((f32x4*)grad_out)[i] = g;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float mj = m[j], vj = v[j];
      w[j] = upd(w[j], g[j], mj, vj);
      m[j] = mj;
      v[j] = vj;
    }
    ((f32x4*)c.param)[i] = w;
    ((f32x4*)c.exp_avg)[i] = m;
    ((f32x4*)c.exp_avg_sq)[i] = v;
  }
  for (int i = n4 * 4 + threadIdx.x; i < c.n; i += 256) {
    float m = c.exp_avg[i], v = c.exp_avg_sq[i];
    float g = c.grad[i];
    if (CLIP) {
      g = __fmul_rn(g, coef);
      if (write_grad) grad_out[i] = g;
    }
    c.param[i] = upd(c.param[i], g, m, v);
    c.exp_avg[i] = m;
    c.exp_avg_sq[i] = v;
  }
}

__global__ __launch_bounds__(256) void adam_l2_multi_kernel(const tsr_adam_chunk* __restrict__ chunks, float lr,
                                                            float b1, float b2, float omb1, float omb2, float eps,
                                                            float wd, float bc1, float bc2_sqrt) {
  adam_l2_multi_body<false>(chunks, lr, b1, b2, omb1, omb2, eps, wd, bc1, bc2_sqrt, nullptr);
}

// hyper = {lr, bc1, bc2_sqrt} in device memory: a captured graph replays this launch with the values written before
// each replay instead of the ones of the capture.
__global__ __launch_bounds__(256) void adam_l2_multi_dev_kernel(const tsr_adam_chunk* __restrict__ chunks,
                                                                const float* __restrict__ hyper, float b1, float b2,
                                                                float omb1, float omb2, float eps, float wd) {
  adam_l2_multi_body<false>(chunks, hyper[0], b1, b2, omb1, omb2, eps, wd, hyper[1], hyper[2], nullptr);
}

// The clipping forms of the two kernels above: clip[0] is the coefficient tsr_grad_norm_multi wrote.
__global__ __launch_bounds__(256) void adam_l2_multi_clip_kernel(const tsr_adam_chunk* __restrict__ chunks, float lr,
                                                                 float b1, float b2, float omb1, float omb2, float eps,
                                                                 float wd, float bc1, float bc2_sqrt,
                                                                 const float* __restrict__ clip) {
  adam_l2_multi_body<true>(chunks, lr, b1, b2, omb1, omb2, eps, wd, bc1, bc2_sqrt, clip);
}

__global__ __launch_bounds__(256) void adam_l2_multi_dev_clip_kernel(const tsr_adam_chunk* __restrict__ chunks,
                                                                     const float* __restrict__ hyper, float b1,
                                                                     float b2, float omb1, float omb2, float eps,
                                                                     float wd, const float* __restrict__ clip) {
  adam_l2_multi_body<true>(chunks, hyper[0], b1, b2, omb1, omb2, eps, wd, hyper[1], hyper[2], clip);
}

// The per-step scalars of both launch forms, formed on the host exactly one way.  betas arrive as doubles and every
// derived constant is formed in double like torch does on the host: (1.f - 0.999f) is 1.3e-5 off 0.001
static void adam_hyper(float lr, double beta1, double beta2, int step, float* out3) {
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  out3[0] = lr;
  out3[1] = (float)bc1;
  out3[2] = (float)sqrt(bc2);
}

extern "C" int tsr_adam_hyper(float lr, double beta1, double beta2, int step, float* out3) {
  if (!out3 || step <= 0) return TSR_ERR_ARG;
  adam_hyper(lr, beta1, beta2, step, out3);
  return TSR_OK;
}

extern "C" int tsr_adam_l2_multi(const tsr_adam_chunk* chunks, int n_chunks, float lr, double beta1, double beta2,
                                 float eps, float weight_decay, int step, void* stream) {
  if (!chunks || n_chunks <= 0 || step <= 0) return TSR_ERR_ARG;
  float h[3];
  adam_hyper(lr, beta1, beta2, step, h);
  hipLaunchKernelGGL(adam_l2_multi_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, chunks, h[0], (float)beta1,
                     (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, weight_decay, h[1], h[2]);
  return tsr_check_launch();
}

extern "C" int tsr_adam_l2_multi_dev(const tsr_adam_chunk* chunks, int n_chunks, const float* hyper, double beta1,
                                     double beta2, float eps, float weight_decay, void* stream) {
  if (!chunks || n_chunks <= 0 || !hyper) return TSR_ERR_ARG;
  hipLaunchKernelGGL(adam_l2_multi_dev_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, chunks, hyper,
                     (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, weight_decay);
  return tsr_check_launch();
}

extern "C" int tsr_adam_l2_multi_clip(const tsr_adam_chunk* chunks, int n_chunks, float lr, double beta1,
                                      double beta2, float eps, float weight_decay, int step, const float* clip,
                                      void* stream) {
  if (!chunks || n_chunks <= 0 || step <= 0 || !clip) return TSR_ERR_ARG;
  float h[3];
  adam_hyper(lr, beta1, beta2, step, h);
  hipLaunchKernelGGL(adam_l2_multi_clip_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, chunks, h[0],
                     (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, weight_decay, h[1],
                     h[2], clip);
  return tsr_check_launch();
}

extern "C" int tsr_adam_l2_multi_dev_clip(const tsr_adam_chunk* chunks, int n_chunks, const float* hyper,
                                          double beta1, double beta2, float eps, float weight_decay, const float* clip,
                                          void* stream) {
  if (!chunks || n_chunks <= 0 || !hyper || !clip) return TSR_ERR_ARG;
  hipLaunchKernelGGL(adam_l2_multi_dev_clip_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, chunks, hyper,
                     (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, weight_decay, clip);
  return tsr_check_launch();
}

// ------------------------------------------------------------------------------------------
// Global L2 norm of the gradients a chunk table points at, and torch's clip coefficient (torch.nn.utils.
// clip_grad_norm_, cpu/trainer.py:356): deterministic, no float atomics.  Workgroup b walks chunks b, b + GN_BLOCKS,
// ...: each thread squares and sums its (<= 16) elements of a chunk in fp32 with 16-B loads and adds that to a double
// accumulator; the workgroup combines its threads in a fixed tree into part[b].  One workgroup then sums the partials
// in a fixed tree and forms {total_norm, clip_coef}.
// ------------------------------------------------------------------------------------------
#define GN_BLOCKS 256      // partials of tsr_grad_norm_multi (its work buffer holds GN_BLOCKS doubles)

__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const tsr_adam_chunk* __restrict__ chunks,
                                                                int n_chunks, double* __restrict__ part) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int b = blockIdx.x; b < n_chunks; b += gridDim.x) {
    const tsr_adam_chunk c = chunks[b];
    float cs = 0.f;
    const int n4 = (((size_t)c.grad & 15) == 0) ? (c.n >> 2) : 0;
    for (int i = threadIdx.x; i < n4; i += 256) {
      const f32x4 g = ((const f32x4*)c.grad)[i];
      cs = fmaf(g[0], g[0], cs);
      cs = fmaf(g[1], g[1], cs);
      cs = fmaf(g[2], g[2], cs);
      cs = fmaf(g[3], g[3], cs);
    }
    for (int i = n4 * 4 + threadIdx.x; i < c.n; i += 256) cs = fmaf(c.grad[i], c.grad[i], cs);
    s += (double)cs;
  }
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (threadIdx.x < k) sh[threadIdx.x] += sh[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

__global__ __launch_bounds__(GN_BLOCKS) void grad_norm_final_kernel(const double* __restrict__ part, float max_norm,
                                                                    float* __restrict__ out2) {
  __shared__ double sh[GN_BLOCKS];
  sh[threadIdx.x] = part[threadIdx.x];
  __syncthreads();
  for (int k = GN_BLOCKS / 2; k > 0; k >>= 1) {
    if (threadIdx.x < k) sh[threadIdx.x] += sh[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(sh[0]);
    // torch: clip_coef = max_norm / (total_norm + 1e-6) is Tensor.__rdiv__ = (total_norm + 1e-6).reciprocal() *
    // max_norm, all fp32; then clamp(max=1.0), which keeps a NaN (fminf would not)
    const float coef = __fmul_rn(1.0f / __fadd_rn(norm, 1e-6f), max_norm);
    out2[0] = norm;
    out2[1] = coef > 1.0f ? 1.0f : coef;
  }
}

extern "C" int tsr_grad_norm_multi(const tsr_adam_chunk* chunks, int n_chunks, float max_norm, double* work,
                                   float* out2, void* stream) {
  if (!chunks || n_chunks <= 0 || !work || !out2) return TSR_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(grad_norm_partial_kernel, dim3(GN_BLOCKS), dim3(256), 0, st, chunks, n_chunks, work);
  hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(GN_BLOCKS), 0, st, work, max_norm, out2);
  return tsr_check_launch();
}

// ------------------------------------------------------------------------------------------
// Welford batch statistics of a CB16 channel slice (for the VALU stem, which has no stats
// epilogue): entry = (image, 64-pixel chunk); slab/slab_cnt in the tsr_conv2d_ex epi_mode-1 format.
// ------------------------------------------------------------------------------------------
template <bool B16>
__global__ __launch_bounds__(256) void cb16_stats_kernel(const float* __restrict__ z, int z_ctot, int z_coff,
                                                         int HW, int chunks, float* __restrict__ slab,
                                                         float* __restrict__ slab_cnt) {
  __shared__ float sh[256 * 3];
  const int tid = threadIdx.x, c = tid & 63, pg = tid >> 6;
  const int e = blockIdx.x, b = e / chunks, ch = e - b * chunks;
  const int oc = z_coff + c;
  const size_t zo = (((size_t)b * (z_ctot >> 4) + (oc >> 4)) * HW) * 16 + (oc & 15);
  float v[16];
  float cnt = 0.f, sum = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int p = ch * 64 + pg * 16 + k;
    v[k] = 0.f;
    if (p < HW) { v[k] = tsr_ld1<B16>(z, zo + (size_t)p * 16); cnt += 1.f; sum += v[k]; }
  }
  const float mean = cnt > 0.f ? sum / cnt : 0.f;
  float m2 = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int p = ch * 64 + pg * 16 + k;
    if (p < HW) { const float d = v[k] - mean; m2 = fmaf(d, d, m2); }
  }
  sh[tid * 3] = cnt; sh[tid * 3 + 1] = mean; sh[tid * 3 + 2] = m2;
  __syncthreads();
  if (pg == 0) {
    float n = cnt, mu = mean, M = m2;
    for (int k = 1; k < 4; ++k) {
      const float n2 = sh[(k * 64 + c) * 3], mu2 = sh[(k * 64 + c) * 3 + 1], M2 = sh[(k * 64 + c) * 3 + 2];
      const float nt = n + n2;
      if (nt > 0.f) {
        const float d = mu2 - mu;
        M = M + M2 + d * d * (n * n2 / nt);
        mu = mu + d * (n2 / nt);
      }
      n = nt;
    }
    slab[((size_t)e * 64 + c) * 2] = mu;
    slab[((size_t)e * 64 + c) * 2 + 1] = M;
    if (c == 0) slab_cnt[e] = n;
  }
}

extern "C" int tsr_cb16_stats_entries(int B, int HW) { return B * ((HW + 63) / 64); }

extern "C" int tsr_cb16_stats(const float* z, int z_ctot, int z_coff, int B, int HW, float* slab, float* slab_cnt,
                              void* stream) {
  if (!z || !slab || !slab_cnt || (z_ctot & 15) || (z_coff & 15) || z_coff + 64 > z_ctot || B <= 0) return TSR_ERR_ARG;
  const int chunks = (HW + 63) / 64;
  hipLaunchKernelGGL(cb16_stats_kernel<false>, dim3(B * chunks), dim3(256), 0, (hipStream_t)stream, z, z_ctot, z_coff, HW,
                     chunks, slab, slab_cnt);
  return tsr_check_launch();
}

// z is a bf16 CB16 tensor (training with bf16 activation storage: the stem's stored pre-activation)
extern "C" int tsr_cb16_stats_b16(const void* z, int z_ctot, int z_coff, int B, int HW, float* slab, float* slab_cnt,
                                  void* stream) {
  if (!z || !slab || !slab_cnt || (z_ctot & 15) || (z_coff & 15) || z_coff + 64 > z_ctot || B <= 0) return TSR_ERR_ARG;
  const int chunks = (HW + 63) / 64;
  hipLaunchKernelGGL(cb16_stats_kernel<true>, dim3(B * chunks), dim3(256), 0, (hipStream_t)stream, (const float*)z, z_ctot,
                     z_coff, HW, chunks, slab, slab_cnt);
  return tsr_check_launch();
}

// ------------------------------------------------------------------------------------------
// Per-sample PSNR / SSIM of eval_func (train/tactileSR_train.py:87-94; utility/tools.py:49-81).
//   PSNR = 10 log10(max^2 / (sum (a-b)^2 / psnr_div)),  psnr_div = shape[0]*shape[1] of the tensor the
//   reference passes ((1,H,W) in eval_func -> H: the reference's /40 quirk; (H,W) -> H*W).
//   SSIM = single global window with C1, C2.
// One workgroup per sample, fp64 accumulation.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void psnr_ssim_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                        int n, double psnr_div, double maxv, double C1, double C2,
                                                        float* __restrict__ psnr, float* __restrict__ ssim) {
  __shared__ double sh[256 * 6];
  const float* pa = a + (size_t)blockIdx.x * n;
  const float* pb = b + (size_t)blockIdx.x * n;
  double s[6] = {0, 0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < n; i += 256) {
    const double x = pa[i], y = pb[i];
    s[0] += (x - y) * (x - y); s[1] += x; s[2] += y; s[3] += x * x; s[4] += y * y; s[5] += x * y;
  }
  for (int k = 0; k < 6; ++k) sh[threadIdx.x * 6 + k] = s[k];
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (threadIdx.x < st)
      for (int k = 0; k < 6; ++k) sh[threadIdx.x * 6 + k] += sh[(threadIdx.x + st) * 6 + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double mse = sh[0] / psnr_div;
    psnr[blockIdx.x] = (float)(10.0 * log10(maxv * maxv / mse));
    const double mu1 = sh[1] / n, mu2 = sh[2] / n;
    const double s1 = sh[3] / n - mu1 * mu1, s2 = sh[4] / n - mu2 * mu2, s12 = sh[5] / n - mu1 * mu2;
    ssim[blockIdx.x] = (float)(((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2)));
  }
}

extern "C" int tsr_psnr_ssim(const float* a, const float* b, int B, int n, double psnr_div, double max_value,
                             double C1, double C2, float* psnr, float* ssim, void* stream) {
  if (!a || !b || !psnr || !ssim || B <= 0 || n <= 0 || psnr_div <= 0) return TSR_ERR_ARG;
  hipLaunchKernelGGL(psnr_ssim_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, a, b, n, psnr_div, max_value, C1,
                     C2, psnr, ssim);
  return tsr_check_launch();
}
