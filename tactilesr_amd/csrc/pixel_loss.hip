// Pixel losses of the train step: MSE, L1, Charbonnier and Huber of d = y - t with an optional contact weight, value and
// gradients from one pass (tsr_pixel_loss_fwd_bwd, include/tactilesr_hip.h).
//
//   w_p  = 1 + fg_weight [t_p > fg_threshold]            (fp32 comparison; a NaN target compares false)
//   loss = (1/n) sum_p w_p rho(d_p),   g_p = w_p rho'(d_p) / n,   dy (+)= dy_scale g,   dt = -dy_scale g
//
// d, rho, rho' and the coefficient dy_scale w / n are fp64; the value and every gradient element are rounded to fp32
// once, at the store.  The sum is fp64 in a fixed order: each thread over its grid-stride elements, a wave64 by
// shuffles, the workgroup's four waves through LDS, one partial per workgroup into `work`, and a second one-workgroup
// launch over the partials.  No atomics and no completion counter: two launches give the same bits.
//
// A streaming kernel: every element is read once (y, t, and dy when it accumulates) and written once per gradient.
// Where y, t, dy and dt (those given) share one offset from 16-byte alignment, the first workgroup takes the up to three
// elements in front of the first aligned one and the up to three behind the last whole float4 one by one, and the body
// moves as float4, two per thread and stride, all loads issued before the first store.  Pointers at different offsets
// take the same loop one float at a time (consecutive lanes still cover consecutive dwords).
#include "tsr_common.h"
#include "tactilesr_hip.h"

namespace {

constexpr int PXL_THREADS = 256;
constexpr int PXL_WAVES = PXL_THREADS / 64;
constexpr int PXL_MAX_WGS = 2048;          // 8 per CU on 256 CUs; == TSR_PIXEL_LOSS_WORK

struct pxl_params {
  double p;        // Charbonnier: eps^2; Huber: delta
  double w1;       // the contact pixel's weight 1 + fg_weight
  double c0, c1;   // dy_scale / n and dy_scale (1 + fg_weight) / n
  float thr;
  int has_dy, accumulate, has_dt;
};

// One element: adds w rho(d) to acc, returns dy_scale w rho'(d) / n.
template <int KIND>
__device__ __forceinline__ double pxl_elem(float yf, float tf, const pxl_params& q, double& acc) {
  const double d = (double)yf - (double)tf;
  const bool fg = tf > q.thr;
  const double w = fg ? q.w1 : 1.0, c = fg ? q.c1 : q.c0;
  double rho, gp;
  if constexpr (KIND == 0) {
    rho = d * d;
    gp = 2.0 * d;
  } else if constexpr (KIND == 1) {
    rho = fabs(d);
    gp = d > 0 ? 1.0 : (d < 0 ? -1.0 : d);                 // sign(0) = 0; a NaN stays a NaN
  } else if constexpr (KIND == 2) {
    rho = sqrt(fma(d, d, q.p));
    gp = d / rho;                                          // +-Inf: Inf / Inf = NaN
  } else {
    const double a = fabs(d);
    if (a <= q.p) {
      rho = 0.5 * d * d;
      gp = d;
    } else {                                               // a NaN lands here: rho and gp are NaN
      rho = q.p * (a - 0.5 * q.p);
      gp = d > 0 ? q.p : (d < 0 ? -q.p : d);
    }
  }
  acc = fma(w, rho, acc);
  return c * gp;
}

__device__ __forceinline__ float pxl_dy(double g, float old, int accumulate) {
  return accumulate ? (float)((double)old + g) : (float)g;
}

template <int KIND>
__device__ __forceinline__ void pxl_scalar(const float* y, const float* t, float* dy, float* dt, size_t i,
                                           const pxl_params& q, double& acc) {
  const double g = pxl_elem<KIND>(y[i], t[i], q, acc);
  if (q.has_dy) dy[i] = pxl_dy(g, q.accumulate ? dy[i] : 0.f, q.accumulate);
  if (q.has_dt) dt[i] = (float)(-g);
}

template <int KIND>
__device__ __forceinline__ void pxl_vec4(const float4& a, const float4& b, float4& o, float4& ot, const pxl_params& q,
                                         double& acc) {
  const double g0 = pxl_elem<KIND>(a.x, b.x, q, acc), g1 = pxl_elem<KIND>(a.y, b.y, q, acc);
  const double g2 = pxl_elem<KIND>(a.z, b.z, q, acc), g3 = pxl_elem<KIND>(a.w, b.w, q, acc);
  o = make_float4(pxl_dy(g0, o.x, q.accumulate), pxl_dy(g1, o.y, q.accumulate), pxl_dy(g2, o.z, q.accumulate),
                  pxl_dy(g3, o.w, q.accumulate));
  ot = make_float4((float)(-g0), (float)(-g1), (float)(-g2), (float)(-g3));
}

// Fixed-order sum over the workgroup; thread 0 holds the total.
__device__ __forceinline__ double pxl_block_sum(double v, double* sh) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0;
  if (threadIdx.x == 0)
    for (int k = 0; k < PXL_WAVES; ++k) s += sh[k];
  return s;
}

// head: the scalar elements in front of the body (VEC only); nbody: float4 (VEC) or float (!VEC) items of the body.
template <int KIND, bool VEC>
__global__ __launch_bounds__(PXL_THREADS) void pixel_loss_kernel(const float* y, const float* t, float* dy, float* dt,
                                                                 size_t n, int head, size_t nbody, pxl_params q,
                                                                 double* __restrict__ part) {
  __shared__ double sh[PXL_WAVES];
  double acc = 0;
  const size_t tid = (size_t)blockIdx.x * PXL_THREADS + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * PXL_THREADS;
  if constexpr (VEC) {
    const float4* y4 = reinterpret_cast<const float4*>(y + head);
    const float4* t4 = reinterpret_cast<const float4*>(t + head);
    float4* dy4 = reinterpret_cast<float4*>(dy + head);      // not dereferenced when dy / dt is NULL
    float4* dt4 = reinterpret_cast<float4*>(dt + head);
    size_t v = tid;
    for (; v + stride < nbody; v += 2 * stride) {
      const size_t u = v + stride;
      const float4 a0 = y4[v], b0 = t4[v], a1 = y4[u], b1 = t4[u];
      float4 o0 = make_float4(0.f, 0.f, 0.f, 0.f), o1 = o0, p0, p1;
      if (q.accumulate) {
        o0 = dy4[v];
        o1 = dy4[u];
      }
      pxl_vec4<KIND>(a0, b0, o0, p0, q, acc);
      pxl_vec4<KIND>(a1, b1, o1, p1, q, acc);
      if (q.has_dy) {
        dy4[v] = o0;
        dy4[u] = o1;
      }
      if (q.has_dt) {
        dt4[v] = p0;
        dt4[u] = p1;
      }
    }
    if (v < nbody) {
      const float4 a0 = y4[v], b0 = t4[v];
      float4 o0 = make_float4(0.f, 0.f, 0.f, 0.f), p0;
      if (q.accumulate) o0 = dy4[v];
      pxl_vec4<KIND>(a0, b0, o0, p0, q, acc);
      if (q.has_dy) dy4[v] = o0;
      if (q.has_dt) dt4[v] = p0;
    }
    if (blockIdx.x == 0) {                                   // at most 3 + 3 elements outside the body
      const size_t after = (size_t)head + 4 * nbody;
      if ((int)threadIdx.x < head) pxl_scalar<KIND>(y, t, dy, dt, threadIdx.x, q, acc);
      if (after + threadIdx.x < n) pxl_scalar<KIND>(y, t, dy, dt, after + threadIdx.x, q, acc);
    }
  } else {
    for (size_t i = tid; i < nbody; i += stride) pxl_scalar<KIND>(y, t, dy, dt, i, q, acc);
  }
  const double s = pxl_block_sum(acc, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// loss = (sum of the nb <= PXL_MAX_WGS partials) / n: thread k adds partials k, k + 256, ... in order, then the
// workgroup sum.
__global__ __launch_bounds__(PXL_THREADS) void pixel_loss_final_kernel(const double* __restrict__ part, int nb,
                                                                       double inv_n, float* __restrict__ loss) {
  __shared__ double sh[PXL_WAVES];
  double acc = 0;
  for (int k = threadIdx.x; k < nb; k += PXL_THREADS) acc += part[k];
  const double s = pxl_block_sum(acc, sh);
  if (threadIdx.x == 0) loss[0] = (float)(s * inv_n);
}

template <int KIND>
void pxl_launch(const float* y, const float* t, float* dy, float* dt, size_t n, const pxl_params& q, double* work,
                float* loss, hipStream_t st) {
  const uintptr_t off = (uintptr_t)y & 15;
  bool vec = ((uintptr_t)y & 3) == 0 && ((uintptr_t)t & 15) == off;
  if (dy) vec = vec && ((uintptr_t)dy & 15) == off;
  if (dt) vec = vec && ((uintptr_t)dt & 15) == off;
  int head = 0;
  size_t nbody = n;
  if (vec) {
    head = (int)(((16 - off) & 15) / 4);
    if ((size_t)head + 4 > n) {                              // not one whole aligned float4: one by one
      vec = false;
      head = 0;
    } else {
      nbody = (n - head) / 4;
    }
  }
  const size_t per_wg = (size_t)PXL_THREADS * (vec ? 2 : 1); // items of the body a workgroup takes per stride
  const size_t wgs = (nbody + per_wg - 1) / per_wg;
  const int nb = (int)(wgs > (size_t)PXL_MAX_WGS ? (size_t)PXL_MAX_WGS : wgs);
  if (vec)
    hipLaunchKernelGGL((pixel_loss_kernel<KIND, true>), dim3(nb), dim3(PXL_THREADS), 0, st, y, t, dy, dt, n, head, nbody,
                       q, work);
  else
    hipLaunchKernelGGL((pixel_loss_kernel<KIND, false>), dim3(nb), dim3(PXL_THREADS), 0, st, y, t, dy, dt, n, head,
                       nbody, q, work);
  hipLaunchKernelGGL(pixel_loss_final_kernel, dim3(1), dim3(PXL_THREADS), 0, st, work, nb, 1.0 / (double)n, loss);
}

// ------------------------------------------------------------------------------------------
// Per-image form (tsr_pixel_loss_ps_fwd_bwd): one workgroup per image, the images walked at a stride of the grid.
// Thread k owns the quads k, k + 256, ... of its image's plane (quad j = elements 4j .. 4j + 3) and adds their terms in
// that order; the workgroup sum is pxl_block_sum.  The order is a function of P alone: neither the grid cap nor the path
// (float4 where P % 4 == 0 and every base is 16-byte aligned, one float at a time otherwise) changes a bit.
// A gradient element is the flat launch's fp64 value for n = B P, times (double)s_b, rounded once; an image whose s_b
// is exactly 1 (or s NULL) runs the flat launch's own expressions.  s_b == 0 skips the image: y and t are not read.
// ------------------------------------------------------------------------------------------
constexpr int PXL_PS_MAX_WGS = 2048;

template <int KIND>
__device__ __forceinline__ void pxl_scalar_scaled(const float* y, const float* t, float* dy, float* dt, size_t i,
                                                  const pxl_params& q, double sd, double& acc) {
  const double g = pxl_elem<KIND>(y[i], t[i], q, acc) * sd;
  if (q.has_dy) dy[i] = pxl_dy(g, q.accumulate ? dy[i] : 0.f, q.accumulate);
  if (q.has_dt) dt[i] = (float)(-g);
}

template <int KIND>
__device__ __forceinline__ void pxl_vec4_scaled(const float4& a, const float4& b, float4& o, float4& ot,
                                                const pxl_params& q, double sd, double& acc) {
  const double g0 = pxl_elem<KIND>(a.x, b.x, q, acc) * sd, g1 = pxl_elem<KIND>(a.y, b.y, q, acc) * sd;
  const double g2 = pxl_elem<KIND>(a.z, b.z, q, acc) * sd, g3 = pxl_elem<KIND>(a.w, b.w, q, acc) * sd;
  o = make_float4(pxl_dy(g0, o.x, q.accumulate), pxl_dy(g1, o.y, q.accumulate), pxl_dy(g2, o.z, q.accumulate),
                  pxl_dy(g3, o.w, q.accumulate));
  ot = make_float4((float)(-g0), (float)(-g1), (float)(-g2), (float)(-g3));
}

// One image's plane; y, t, dy, dt point at its first element.
template <int KIND, bool VEC, bool SCALED>
__device__ __forceinline__ void pxl_ps_plane(const float* y, const float* t, float* dy, float* dt, int P,
                                             const pxl_params& q, double sd, double& acc) {
  const int nq = (P + 3) >> 2;
  if constexpr (VEC) {                                       // P % 4 == 0: every quad is whole
    const float4* y4 = reinterpret_cast<const float4*>(y);
    const float4* t4 = reinterpret_cast<const float4*>(t);
    float4* dy4 = reinterpret_cast<float4*>(dy);             // not dereferenced when dy / dt is NULL
    float4* dt4 = reinterpret_cast<float4*>(dt);
    for (int v = threadIdx.x; v < nq; v += PXL_THREADS) {
      const float4 a0 = y4[v], b0 = t4[v];
      float4 o0 = make_float4(0.f, 0.f, 0.f, 0.f), p0;
      if (q.accumulate) o0 = dy4[v];
      if constexpr (SCALED) pxl_vec4_scaled<KIND>(a0, b0, o0, p0, q, sd, acc);
      else pxl_vec4<KIND>(a0, b0, o0, p0, q, acc);
      if (q.has_dy) dy4[v] = o0;
      if (q.has_dt) dt4[v] = p0;
    }
  } else {
    for (int v = threadIdx.x; v < nq; v += PXL_THREADS) {
      const int i0 = 4 * v, i1 = min(i0 + 4, P);
      for (int i = i0; i < i1; ++i) {
        if constexpr (SCALED) pxl_scalar_scaled<KIND>(y, t, dy, dt, (size_t)i, q, sd, acc);
        else pxl_scalar<KIND>(y, t, dy, dt, (size_t)i, q, acc);
      }
    }
  }
}

template <int KIND, bool VEC>
__global__ __launch_bounds__(PXL_THREADS) void pixel_loss_ps_kernel(const float* y, const float* t, float* dy, float* dt,
                                                                    const float* __restrict__ s,
                                                                    float* __restrict__ pix, int B, int P,
                                                                    pxl_params q) {
  __shared__ double sh[PXL_WAVES];
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const size_t base = (size_t)b * (size_t)P;
    const float sb = s ? s[b] : 1.f;
    if (sb == 0.f) {                                         // skipped: nothing of the image is read
      if (threadIdx.x == 0) pix[b] = 0.f;
      const bool zero_dy = q.has_dy && !q.accumulate;
      if constexpr (VEC) {
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int v = threadIdx.x; v < (P >> 2); v += PXL_THREADS) {
          if (zero_dy) reinterpret_cast<float4*>(dy + base)[v] = z;
          if (q.has_dt) reinterpret_cast<float4*>(dt + base)[v] = z;
        }
      } else {
        for (int i = threadIdx.x; i < P; i += PXL_THREADS) {
          if (zero_dy) dy[base + i] = 0.f;
          if (q.has_dt) dt[base + i] = 0.f;
        }
      }
      continue;
    }
    const double sd = (double)sb;
    double acc = 0;
    if (sd == 1.0)
      pxl_ps_plane<KIND, VEC, false>(y + base, t + base, dy + base, dt + base, P, q, sd, acc);
    else                                                     // a NaN scale lands here and poisons its own image
      pxl_ps_plane<KIND, VEC, true>(y + base, t + base, dy + base, dt + base, P, q, sd, acc);
    const double tot = pxl_block_sum(acc, sh);
    if (threadIdx.x == 0) pix[b] = (float)(tot / (double)P);
    __syncthreads();                                         // sh is written again for the next image
  }
}

template <int KIND>
void pxl_ps_launch(const float* y, const float* t, float* dy, float* dt, const float* s, float* pix, int B, int P,
                   const pxl_params& q, int max_wgs, hipStream_t st) {
  bool vec = (P & 3) == 0 && ((uintptr_t)y & 15) == 0 && ((uintptr_t)t & 15) == 0;
  if (dy) vec = vec && ((uintptr_t)dy & 15) == 0;
  if (dt) vec = vec && ((uintptr_t)dt & 15) == 0;
  const int nb = B < max_wgs ? B : max_wgs;
  if (vec)
    hipLaunchKernelGGL((pixel_loss_ps_kernel<KIND, true>), dim3(nb), dim3(PXL_THREADS), 0, st, y, t, dy, dt, s, pix, B, P,
                       q);
  else
    hipLaunchKernelGGL((pixel_loss_ps_kernel<KIND, false>), dim3(nb), dim3(PXL_THREADS), 0, st, y, t, dy, dt, s, pix, B,
                       P, q);
}

}  // namespace

extern "C" int tsr_pixel_loss_fwd_bwd(const float* y, const float* t, long long n, int kind, double param,
                                      float fg_weight, float fg_threshold, float* loss, float* dy, float dy_scale,
                                      int accumulate, float* dt, double* work, void* stream) {
  if (!y || !t || !loss || !work || n <= 0) return TSR_ERR_ARG;
  if (kind < 0 || kind > 3) return TSR_ERR_ARG;
  if (kind >= 2 && !(param > 0 && param <= 1.79769313486231570e308)) return TSR_ERR_ARG;      // <= 0, NaN, Inf
  if (!(fg_weight >= 0 && fg_weight <= 3.402823466e38f)) return TSR_ERR_ARG;                  // < 0, NaN, Inf
  if (fg_threshold != fg_threshold || dy_scale != dy_scale) return TSR_ERR_ARG;
  if (accumulate != 0 && accumulate != 1) return TSR_ERR_ARG;
  if (accumulate == 1 && !dy) return TSR_ERR_ARG;
  if (dy && dt == dy) return TSR_ERR_ARG;
  static_assert(PXL_MAX_WGS == TSR_PIXEL_LOSS_WORK, "work holds one partial per workgroup");
  pxl_params q;
  q.p = kind == 2 ? param * param : param;
  q.w1 = 1.0 + (double)fg_weight;
  q.c0 = (double)dy_scale / (double)n;
  q.c1 = (double)dy_scale * q.w1 / (double)n;
  q.thr = fg_threshold;
  q.has_dy = dy != nullptr;
  q.accumulate = accumulate;
  q.has_dt = dt != nullptr;
  hipStream_t st = (hipStream_t)stream;
  switch (kind) {
    case 0: pxl_launch<0>(y, t, dy, dt, (size_t)n, q, work, loss, st); break;
    case 1: pxl_launch<1>(y, t, dy, dt, (size_t)n, q, work, loss, st); break;
    case 2: pxl_launch<2>(y, t, dy, dt, (size_t)n, q, work, loss, st); break;
    default: pxl_launch<3>(y, t, dy, dt, (size_t)n, q, work, loss, st); break;
  }
  return tsr_check_launch();
}

extern "C" int tsr_pixel_loss_ps_fwd_bwd_wgs(const float* y, const float* t, int B, long long P, int kind, double param,
                                             float fg_weight, float fg_threshold, const float* s, float* pix, float* dy,
                                             float dy_scale, int accumulate, float* dt, int max_wgs, void* stream) {
  if (!y || !t || !pix || B <= 0 || P <= 0 || P > (1LL << 28) || max_wgs < 1) return TSR_ERR_ARG;
  if (kind < 0 || kind > 3) return TSR_ERR_ARG;
  if (kind >= 2 && !(param > 0 && param <= 1.79769313486231570e308)) return TSR_ERR_ARG;      // <= 0, NaN, Inf
  if (!(fg_weight >= 0 && fg_weight <= 3.402823466e38f)) return TSR_ERR_ARG;                  // < 0, NaN, Inf
  if (fg_threshold != fg_threshold || dy_scale != dy_scale) return TSR_ERR_ARG;
  if (accumulate != 0 && accumulate != 1) return TSR_ERR_ARG;
  if (accumulate == 1 && !dy) return TSR_ERR_ARG;
  if (dy && dt == dy) return TSR_ERR_ARG;
  static_assert(PXL_PS_MAX_WGS == TSR_PIXEL_LOSS_PS_MAX_WGS, "the default grid cap of the header");
  const double n = (double)((long long)B * P);               // the flat launch's divisor for the same batch
  pxl_params q;
  q.p = kind == 2 ? param * param : param;
  q.w1 = 1.0 + (double)fg_weight;
  q.c0 = (double)dy_scale / n;
  q.c1 = (double)dy_scale * q.w1 / n;
  q.thr = fg_threshold;
  q.has_dy = dy != nullptr;
  q.accumulate = accumulate;
  q.has_dt = dt != nullptr;
  hipStream_t st = (hipStream_t)stream;
  switch (kind) {
    case 0: pxl_ps_launch<0>(y, t, dy, dt, s, pix, B, (int)P, q, max_wgs, st); break;
    case 1: pxl_ps_launch<1>(y, t, dy, dt, s, pix, B, (int)P, q, max_wgs, st); break;
    case 2: pxl_ps_launch<2>(y, t, dy, dt, s, pix, B, (int)P, q, max_wgs, st); break;
    default: pxl_ps_launch<3>(y, t, dy, dt, s, pix, B, (int)P, q, max_wgs, st); break;
  }
  return tsr_check_launch();
}

extern "C" int tsr_pixel_loss_ps_fwd_bwd(const float* y, const float* t, int B, long long P, int kind, double param,
                                         float fg_weight, float fg_threshold, const float* s, float* pix, float* dy,
                                         float dy_scale, int accumulate, float* dt, void* stream) {
  return tsr_pixel_loss_ps_fwd_bwd_wgs(y, t, B, P, kind, param, fg_weight, fg_threshold, s, pix, dy, dy_scale, accumulate,
                                       dt, PXL_PS_MAX_WGS, stream);
}
