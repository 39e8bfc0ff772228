// Degradation-consistency loss: the SR image pooled back onto the 4x4 taxels by the sensor model's Gaussian masks
// (reference model/tPSFNet.py:129-141, degradation_process, generalised from 100x100 to any H x W <= 128 x 128), the
// squared residual against the measured z-taxels, and its gradients, from one launch (tsr_degrade_fwd_bwd,
// include/tactilesr_hip.h).
//
//   KM = 100/15138,  c_a = 12 + 25 a,  mn = exp(-100/gamma)
//   X(x) = (x + 0.5) 100/H - 0.5,  Y(v) = (v + 0.5) 100/W - 0.5          (the pixel centres of align_corners=False)
//   E_a[x] = exp(-KM (X(x) - c_a)^2 / gamma),  F_c[v] = exp(-KM (Y(v) - c_c)^2 / gamma)
//   k = gain 1e-4 (100/H)(100/W) / (1 - mn)
//   D_ac = k (sum_xv E_a[x] y_xv F_c[v] - mn sum_xv y_xv),  r_ac = D_ac - z_ac,  q = (1/16) sum_ac r_ac^2
//   dq/dy_xv = (2/16) k (sum_ac r_ac E_a[x] F_c[v] - mn sum_ac r_ac),  dq/dz_ac = -(2/16) r_ac
//
// Everything is fp64 from the exact fp32 inputs; a value is rounded to fp32 once, at its store.
//
// One workgroup of 256 threads owns one image (and walks the batch at a stride of the grid).  A thread owns one group of
// four adjacent columns and every rpp-th row, rpp = 256 / ceil(W/4): consecutive threads read consecutive 16 bytes.
//   forward:   P_a[j] += E_a[x] y[x][v_j] over the thread's rows (16 accumulators) and s0 += y; then
//              T_ac = sum_j P_a[j] F_c[v_j], and the 16 + 1 values are summed over the workgroup: a wave64 by shuffles,
//              the four waves through LDS in order.  Threads 0..15 finish D, r and dz; thread 0 q and sum r.
//   gradient:  G_a[j] = sum_c r_ac F_c[v_j] (16 values), then per row  dy = coef (sum_a E_a[x] G_a[j] - mn sum r).
// The gradient does not read y: the image is read once, and dy once more only when it accumulates.
// The forward takes float4 loads when W % 4 == 0 and y is 16-byte aligned, the gradient float4 accesses when W % 4 == 0
// and dy is; every other case moves the same four columns one float at a time through the same arithmetic, so the bits
// do not depend on the path.  No atomics and a fixed order: two launches give the same bits.
#include <math.h>

#include "tsr_common.h"
#include "tactilesr_hip.h"

namespace {

constexpr int DGL_THREADS = 256;
constexpr int DGL_WAVES = DGL_THREADS / 64;
constexpr int DGL_MAX_HW = 128;
constexpr double DGL_KM = 100.0 / 15138.0;

struct dgl_args {
  const float* y;
  const float* z;
  const float* gamma_dev;
  float* lr_deg;
  float* q;
  float* dy;
  float* dz;
  long long z_bstride;
  double gamma_all, gain, dy_scale;
  int B, H, W, accumulate;
  int vec_y, vec_dy;
};

__global__ __launch_bounds__(DGL_THREADS) void degrade_kernel(dgl_args p) {
  __shared__ double sE[4 * DGL_MAX_HW];        // E_a[x] at sE[4 x + a]: a thread reads the four of a row as two 16-byte loads
  __shared__ double sF[4 * DGL_MAX_HW];        // F_c[v] at sF[4 v + c]
  __shared__ double sPart[DGL_WAVES][17];
  __shared__ double sTot[17];
  __shared__ double sR[18];                    // r_ac, then sum r at [16]
  const int tid = threadIdx.x, H = p.H, W = p.W;
  const int ncg = (W + 3) >> 2, rpp = DGL_THREADS / ncg;          // ncg <= 32, rpp >= 8
  const int cg = tid % ncg, row0 = tid / ncg;                     // row0 >= rpp: the thread has no rows
  const int v0 = 4 * cg, nv = min(4, W - v0);
  const bool active = row0 < rpp;
  const float qnan = __int_as_float(0x7fc00000);
  double g_tab = -1.0;                                            // the gamma the tables hold (none yet)

  for (int b = blockIdx.x; b < p.B; b += gridDim.x) {
    const size_t img = (size_t)b * H * W;
    const double gamma = p.gamma_dev ? (double)p.gamma_dev[b] : p.gamma_all;
    if (!(gamma > 0.0 && gamma <= TSR_DEGRADE_GAMMA_MAX)) {       // a bad device gamma: an all-NaN image, nothing else
      if (p.lr_deg && tid < 16) p.lr_deg[(size_t)b * 16 + tid] = qnan;
      if (p.dz && tid < 16) p.dz[(size_t)b * 16 + tid] = qnan;
      if (p.q && tid == 0) p.q[b] = qnan;
      if (p.dy)
        for (int i = tid; i < H * W; i += DGL_THREADS) p.dy[img + i] = qnan;
      continue;                                                   // uniform over the workgroup
    }
    __syncthreads();                                              // the previous image's reads of the tables and sR
    if (gamma != g_tab) {
      for (int i = tid; i < 4 * (H + W); i += DGL_THREADS) {
        const bool isE = i < 4 * H;
        const int j = isE ? i : i - 4 * H, pos = j >> 2, a = j & 3, n = isE ? H : W;
        const double X = ((double)pos + 0.5) * 100.0 / (double)n - 0.5, d = X - (12.0 + 25.0 * a);
        (isE ? sE : sF)[j] = exp(-DGL_KM * d * d / gamma);
      }
      g_tab = gamma;
    }
    __syncthreads();
    const double mn = exp(-100.0 / gamma);
    const double k = p.gain * 1e-4 * (100.0 / (double)H) * (100.0 / (double)W) / (1.0 - mn);

    // ---- forward: the thread's columns over its rows
    double P[4][4], s0 = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int j = 0; j < 4; ++j) P[a][j] = 0.0;
    if (active) {
      const float* py = p.y + img;
#pragma unroll 2
      for (int x = row0; x < H; x += rpp) {
        float yv[4] = {0.f, 0.f, 0.f, 0.f};
        if (p.vec_y) {
          const float4 t = *reinterpret_cast<const float4*>(py + x * W + v0);
          yv[0] = t.x; yv[1] = t.y; yv[2] = t.z; yv[3] = t.w;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (j < nv) yv[j] = py[x * W + v0 + j];
        }
        const double e0 = sE[4 * x], e1 = sE[4 * x + 1], e2 = sE[4 * x + 2], e3 = sE[4 * x + 3];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j < nv) {
            const double v = (double)yv[j];
            P[0][j] = fma(e0, v, P[0][j]); P[1][j] = fma(e1, v, P[1][j]);
            P[2][j] = fma(e2, v, P[2][j]); P[3][j] = fma(e3, v, P[3][j]);
            s0 += v;
          }
        }
      }
    }
    double T[17];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        double t = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (active && j < nv) t = fma(P[a][j], sF[4 * (v0 + j) + c], t);
        T[4 * a + c] = t;
      }
    T[16] = s0;
#pragma unroll
    for (int i = 0; i < 17; ++i) {
      double v = T[i];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
      if ((tid & 63) == 0) sPart[tid >> 6][i] = v;
    }
    __syncthreads();
    if (tid < 17) {
      double s = 0.0;
      for (int w = 0; w < DGL_WAVES; ++w) s += sPart[w][tid];
      sTot[tid] = s;
    }
    __syncthreads();
    if (tid < 16) {
      const double D = k * (sTot[tid] - mn * sTot[16]);
      if (p.lr_deg) p.lr_deg[(size_t)b * 16 + tid] = (float)D;
      if (p.z) {
        const double r = D - (double)p.z[(long long)b * p.z_bstride + tid];
        sR[tid] = r;
        if (p.dz) p.dz[(size_t)b * 16 + tid] = (float)(-p.dy_scale * 0.125 * r);
      }
    }
    if (!p.z) continue;                                           // the forward alone (uniform)
    __syncthreads();
    if (tid == 0) {
      double s2 = 0.0, s1 = 0.0;
      for (int i = 0; i < 16; ++i) {
        s2 = fma(sR[i], sR[i], s2);
        s1 += sR[i];
      }
      p.q[b] = (float)(s2 * 0.0625);
      sR[16] = s1;
    }
    if (!p.dy) continue;                                          // uniform; the loop's first barrier orders sR's reuse
    __syncthreads();

    // ---- gradient: the same thread-to-pixel map
    if (active) {
      const double coef = p.dy_scale * 0.125 * k, mnR = mn * sR[16];
      double G[4][4];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          double t = 0.0;
          if (j < nv) {
#pragma unroll
            for (int c = 0; c < 4; ++c) t = fma(sR[4 * a + c], sF[4 * (v0 + j) + c], t);
          }
          G[a][j] = t;
        }
      float* pd = p.dy + img;
#pragma unroll 2
      for (int x = row0; x < H; x += rpp) {
        const double e0 = sE[4 * x], e1 = sE[4 * x + 1], e2 = sE[4 * x + 2], e3 = sE[4 * x + 3];
        double g[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          g[j] = coef * (fma(e3, G[3][j], fma(e2, G[2][j], fma(e1, G[1][j], e0 * G[0][j]))) - mnR);
        float* dst = pd + x * W + v0;
        if (p.vec_dy) {
          float4 o;
          if (p.accumulate) {
            const float4 old = *reinterpret_cast<const float4*>(dst);
            o = make_float4((float)((double)old.x + g[0]), (float)((double)old.y + g[1]), (float)((double)old.z + g[2]),
                            (float)((double)old.w + g[3]));
          } else {
            o = make_float4((float)g[0], (float)g[1], (float)g[2], (float)g[3]);
          }
          *reinterpret_cast<float4*>(dst) = o;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (j < nv) dst[j] = p.accumulate ? (float)((double)dst[j] + g[j]) : (float)g[j];
        }
      }
    }
  }
}

}  // namespace

extern "C" int tsr_degrade_fwd_bwd_wgs(const float* y, int B, int H, int W, const float* z, long long z_bstride,
                                       const float* gamma_dev, double gamma_all, double gain, float* lr_deg, float* q,
                                       float* dy, float dy_scale, int accumulate, float* dz, int max_wgs, void* stream) {
  if (!y || B <= 0 || H <= 0 || W <= 0 || H > DGL_MAX_HW || W > DGL_MAX_HW) return TSR_ERR_ARG;
  if (!gamma_dev && !(gamma_all > 0 && gamma_all <= TSR_DEGRADE_GAMMA_MAX)) return TSR_ERR_ARG;      // <= 0, NaN, too wide
  if (!(gain >= -1.79769313486231570e308 && gain <= 1.79769313486231570e308)) return TSR_ERR_ARG;    // NaN, Inf
  if (z) {
    if (!q) return TSR_ERR_ARG;
    if (B > 1 && z_bstride < 16) return TSR_ERR_ARG;
  } else if (q || dy || dz || !lr_deg) {
    return TSR_ERR_ARG;
  }
  if (accumulate != 0 && accumulate != 1) return TSR_ERR_ARG;
  if (accumulate == 1 && !dy) return TSR_ERR_ARG;
  if (dy_scale != dy_scale) return TSR_ERR_ARG;
  const size_t n = (size_t)B * H * W;
  if (dy && dy < y + n && y < dy + n) return TSR_ERR_ARG;         // dy overlaps y
  if (max_wgs < 1) return TSR_ERR_ARG;
  dgl_args p;
  p.y = y; p.z = z; p.gamma_dev = gamma_dev; p.lr_deg = lr_deg; p.q = q; p.dy = dy; p.dz = dz;
  p.z_bstride = z_bstride; p.gamma_all = gamma_all; p.gain = gain; p.dy_scale = (double)dy_scale;
  p.B = B; p.H = H; p.W = W; p.accumulate = accumulate;
  p.vec_y = (W % 4 == 0) && ((uintptr_t)y & 15) == 0;
  p.vec_dy = dy && (W % 4 == 0) && ((uintptr_t)dy & 15) == 0;
  const int wgs = B < max_wgs ? B : max_wgs;
  hipLaunchKernelGGL(degrade_kernel, dim3(wgs), dim3(DGL_THREADS), 0, (hipStream_t)stream, p);
  return tsr_check_launch();
}

extern "C" int tsr_degrade_fwd_bwd(const float* y, int B, int H, int W, const float* z, long long z_bstride,
                                   const float* gamma_dev, double gamma_all, double gain, float* lr_deg, float* q,
                                   float* dy, float dy_scale, int accumulate, float* dz, void* stream) {
  return tsr_degrade_fwd_bwd_wgs(y, B, H, W, z, z_bstride, gamma_dev, gamma_all, gain, lr_deg, q, dy, dy_scale,
                                 accumulate, dz, TSR_DEGRADE_MAX_WGS, stream);
}
