// Per-sample supervision weights: the scale vector of a batch and the weighted mean of a per-sample vector
// (tsr_sample_scale, tsr_weighted_mean, include/tactilesr_hip.h).
//
//   valid(w)  = w finite and >= 0
//   D         = sum over the valid w_b, fp64, in index order
//   s_b       = invalid ? NaN : mode 0 ("sum")   (D == 0 ? 0 : fl32(w_b B / D))
//                               mode 1 ("batch")  w_b
//   mean      = fl32((1/B) sum_{s_b != 0} s_b v_b), fp64, in index order; v_b is not read where s_b == 0
//
// Both are one workgroup: B is a batch size, and the sum's order is part of the contract.  The workgroup stages a chunk
// of terms in LDS (every thread loads and classifies), thread 0 adds the chunk in index order, and the next chunk
// follows; the only serial work is one fp64 add per sample on operands that are already on chip.
#include "tsr_common.h"
#include "tactilesr_hip.h"

namespace {

constexpr int SW_THREADS = 256;
constexpr int SW_CHUNK = 2048;            // terms staged per pass: 16 KB of LDS

__device__ __forceinline__ bool sw_valid(float w) { return w >= 0.f && w <= 3.402823466e38f; }      // NaN compares false

__global__ __launch_bounds__(SW_THREADS) void sample_scale_kernel(const float* __restrict__ w, int B, int mode,
                                                                  float* __restrict__ s, float* __restrict__ stats) {
  __shared__ double term[SW_CHUNK];
  __shared__ int cnt[SW_THREADS];
  __shared__ double total;
  double D = 0;
  int positive = 0;
  for (int c0 = 0; c0 < B; c0 += SW_CHUNK) {
    const int nc = min(SW_CHUNK, B - c0);
    for (int i = threadIdx.x; i < nc; i += SW_THREADS) {
      const float v = w[c0 + i];
      term[i] = sw_valid(v) ? (double)v : 0.0;               // + 0.0 leaves the sum as it is
      positive += sw_valid(v) && v > 0.f;
    }
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < nc; ++i) D += term[i];
    __syncthreads();
  }
  cnt[threadIdx.x] = positive;
  if (threadIdx.x == 0) total = D;
  __syncthreads();
  for (int k = SW_THREADS / 2; k > 0; k >>= 1) {             // integers: any order
    if ((int)threadIdx.x < k) cnt[threadIdx.x] += cnt[threadIdx.x + k];
    __syncthreads();
  }
  D = total;
  if (threadIdx.x == 0) {
    stats[0] = (float)D;
    stats[1] = (float)cnt[0];
  }
  const float nan = __uint_as_float(0x7fc00000u);
  for (int i = threadIdx.x; i < B; i += SW_THREADS) {
    const float v = w[i];
    float o;
    if (!sw_valid(v)) o = nan;
    else if (mode == 1) o = v;
    else o = D == 0 ? 0.f : (float)(((double)v * (double)B) / D);
    s[i] = o;
  }
}

__global__ __launch_bounds__(SW_THREADS) void weighted_mean_kernel(const float* __restrict__ v,
                                                                   const float* __restrict__ s, int B,
                                                                   float* __restrict__ out) {
  __shared__ double term[SW_CHUNK];
  double acc = 0;
  for (int c0 = 0; c0 < B; c0 += SW_CHUNK) {
    const int nc = min(SW_CHUNK, B - c0);
    for (int i = threadIdx.x; i < nc; i += SW_THREADS) {
      double x = 0.0;
      if (!s) {
        x = (double)v[c0 + i];
      } else {
        const float sb = s[c0 + i];
        if (sb != 0.f) x = (double)sb * (double)v[c0 + i];   // a skipped entry is not read (a NaN s_b is != 0)
      }
      term[i] = x;
    }
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < nc; ++i) acc += term[i];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)(acc / (double)B);
}

}  // namespace

extern "C" int tsr_sample_scale(const float* w, int B, int mode, float* s, float* stats, void* stream) {
  if (!w || !s || !stats || B <= 0 || (mode != 0 && mode != 1)) return TSR_ERR_ARG;
  hipLaunchKernelGGL(sample_scale_kernel, dim3(1), dim3(SW_THREADS), 0, (hipStream_t)stream, w, B, mode, s, stats);
  return tsr_check_launch();
}

extern "C" int tsr_weighted_mean(const float* v, const float* s, int B, float* out, void* stream) {
  if (!v || !out || B <= 0) return TSR_ERR_ARG;
  hipLaunchKernelGGL(weighted_mean_kernel, dim3(1), dim3(SW_THREADS), 0, (hipStream_t)stream, v, s, B, out);
  return tsr_check_launch();
}
