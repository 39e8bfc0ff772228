// Weight averaging (EMA / SWA) over every tensor of a state dict in ONE launch: tsr_ema_multi / tsr_ema_multi_dev
// (include/tactilesr_hip.h).  The launch shape is the fused Adam step's (train_ops.hip, adam_l2_multi_body): block b
// owns chunk record b, <= 4096 contiguous 4-byte words of one tensor.
#include "tsr_common.h"
#include "tactilesr_hip.h"

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

#define EMA_UPDATE 0
#define EMA_STORE 1
#define EMA_LOAD 2
#define EMA_SWAP 3

// The body is shared by both launch forms: omd (= 1 - decay) as a kernel argument (tsr_ema_multi) or read from device
// memory (tsr_ema_multi_dev, the graph-captured step).  avg and src carry no __restrict__: a frozen tensor's record may
// name the same words twice.  Every element is read before it is written and by one thread only, so aliasing (and the
// exchange of SWAP) needs no barrier.  Copies move raw words, so NaN payloads and integer buffers survive bit for bit.
__device__ __forceinline__ void ema_multi_body(const tsr_ema_chunk* __restrict__ chunks, int op, float omd) {
  const tsr_ema_chunk c = chunks[blockIdx.x];
  if (c.n < 1 || c.n > 4096 || c.mode < 0 || c.mode > 1) return;      // a bad record: nothing read, nothing written
  const int kind = (op == EMA_UPDATE && c.mode == 1) ? EMA_STORE : op;      // uniform per workgroup
  const bool vec = ((((size_t)c.avg | (size_t)c.src) & 15) == 0);
  const int n4 = vec ? (c.n >> 2) : 0;
  if (kind == EMA_UPDATE) {
    for (int i = threadIdx.x; i < n4; i += 256) {
      f32x4 a = ((const f32x4*)c.avg)[i];
      const f32x4 s = ((const f32x4*)c.src)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] = fmaf(omd, __fsub_rn(s[j], a[j]), a[j]);
      ((f32x4*)c.avg)[i] = a;
    }
    for (int i = n4 * 4 + threadIdx.x; i < c.n; i += 256) {
      const float a = c.avg[i];
      c.avg[i] = fmaf(omd, __fsub_rn(c.src[i], a), a);
    }
    return;
  }
  unsigned int* avg = (unsigned int*)c.avg;
  unsigned int* src = (unsigned int*)c.src;
  if (kind == EMA_SWAP) {
    for (int i = threadIdx.x; i < n4; i += 256) {
      const u32x4 a = ((const u32x4*)avg)[i], s = ((const u32x4*)src)[i];
      ((u32x4*)avg)[i] = s;
      ((u32x4*)src)[i] = a;
    }
    for (int i = n4 * 4 + threadIdx.x; i < c.n; i += 256) {
      const unsigned int a = avg[i], s = src[i];
      avg[i] = s;
      src[i] = a;
    }
    return;
  }
  unsigned int* dst = kind == EMA_STORE ? avg : src;
  const unsigned int* from = kind == EMA_STORE ? src : avg;
  for (int i = threadIdx.x; i < n4; i += 256) ((u32x4*)dst)[i] = ((const u32x4*)from)[i];
  for (int i = n4 * 4 + threadIdx.x; i < c.n; i += 256) dst[i] = from[i];
}

__global__ __launch_bounds__(256) void ema_multi_kernel(const tsr_ema_chunk* __restrict__ chunks, int op, float omd) {
  ema_multi_body(chunks, op, omd);
}

// omd in device memory: a captured graph replays this launch with the value written before each replay instead of the
// one of the capture (a decay that warms up per step).
__global__ __launch_bounds__(256) void ema_multi_dev_kernel(const tsr_ema_chunk* __restrict__ chunks, int op,
                                                            const float* __restrict__ omd) {
  ema_multi_body(chunks, op, omd[0]);
}

static int ema_args_bad(const tsr_ema_chunk* chunks, int n_chunks, int op) {
  return !chunks || n_chunks <= 0 || op < EMA_UPDATE || op > EMA_SWAP;
}

extern "C" int tsr_ema_multi(const tsr_ema_chunk* chunks, int n_chunks, int op, float one_minus_decay, void* stream) {
  if (ema_args_bad(chunks, n_chunks, op) || !(one_minus_decay >= 0.f && one_minus_decay <= 1.f)) return TSR_ERR_ARG;
  hipLaunchKernelGGL(ema_multi_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, chunks, op, one_minus_decay);
  return tsr_check_launch();
}

extern "C" int tsr_ema_multi_dev(const tsr_ema_chunk* chunks, int n_chunks, int op, const float* one_minus_decay_dev,
                                 void* stream) {
  if (ema_args_bad(chunks, n_chunks, op) || !one_minus_decay_dev) return TSR_ERR_ARG;
  hipLaunchKernelGGL(ema_multi_dev_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, chunks, op,
                     one_minus_decay_dev);
  return tsr_check_launch();
}
