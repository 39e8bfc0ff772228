// Differentiable SSIM: per-image value and d ssim / d prediction from one launch (tsr_ssim_fwd_bwd,
// include/tactilesr_hip.h).  Reference: utility/tools.py:66-81 (calculationSSIM, the global form) and :84-114
// (class SSIM, "# ssim loss"); the windowed form is the literature's Gaussian window, valid correlation.
//
// With x = prediction, t = target and G[.] the window average (separable Gaussian, or 1/n over the whole image):
//   mx = G[x], mt = G[t], sxx = G[x^2] - mx^2, stt = G[t^2] - mt^2, sxt = G[xt] - mx mt
//   A1 = 2 mx mt + C1, A2 = 2 sxt + C2, B1 = mx^2 + mt^2 + C1, B2 = sxx + stt + C2, S = A1 A2 / (B1 B2)
//   ssim = mean of S over the N map positions
//   P = dS/dG[x] = 2 mt (A2 - A1)/(B1 B2) - 2 mx S (1/B1 - 1/B2),  Q = dS/dG[x^2] = -S/B2,  R = dS/dG[xt] = 2 A1/(B1 B2)
//   d ssim / d x_p = (1/N) (G^T[P] + 2 x_p G^T[Q] + t_p G^T[R]),   G^T = the adjoint (full) correlation
//
// Every moment, map value and adjoint sum is fp64: the differences G[x^2] - mx^2 cancel, and fp32 misses the 1e-5
// bar on them (measured: 5.7e-5 on the value, 1.5e-4 of the gradient's maximum).  One workgroup owns one image and
// sums in a fixed order (no atomics): two launches give the same bits, and a NaN / Inf stays in its own image.
#include "tsr_common.h"

namespace {

constexpr int SSIM_MAX_WIN = 11;
constexpr int SSIM_MAX_HW = 128;          // windowed form: H, W <= 128
constexpr int SSIM_THREADS = 256;

struct ssim_gauss { double g[SSIM_MAX_WIN]; };

// Fixed-order sum of one double per thread; every thread returns the total.
__device__ __forceinline__ double ssim_block_sum(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int k = SSIM_THREADS / 2; k > 0; k >>= 1) {
    if (threadIdx.x < k) sh[threadIdx.x] += sh[threadIdx.x + k];
    __syncthreads();
  }
  return sh[0];
}

// A skipped image (s_b == 0): value 0, its dy rows 0 on overwrite and untouched on accumulate.
template <bool HAS_DY>
__device__ __forceinline__ void ssim_skip(float* __restrict__ ssim, float* __restrict__ dy, int n, int accumulate) {
  if (threadIdx.x == 0) ssim[blockIdx.x] = 0.f;
  if constexpr (HAS_DY) {
    if (!accumulate) {
      float* pd = dy + (size_t)blockIdx.x * n;
      for (int i = threadIdx.x; i < n; i += SSIM_THREADS) pd[i] = 0.f;
    }
  }
}

// ------------------------------------------------------------------------------------------
// Global form (win = 0): one window per image, g = 1/n.  The five sums and the formula are psnr_ssim_kernel's
// (train_ops.hip), so the value is what tsr_psnr_ssim reports.
// ------------------------------------------------------------------------------------------
template <bool HAS_DY, bool HAS_S>
__global__ __launch_bounds__(SSIM_THREADS) void ssim_global_kernel(const float* __restrict__ y,
                                                                   const float* __restrict__ t, int n, double C1,
                                                                   double C2, float* __restrict__ ssim,
                                                                   float* __restrict__ dy, double dy_scale,
                                                                   int accumulate, const float* __restrict__ scale) {
  __shared__ double sh[SSIM_THREADS * 5];
  if constexpr (HAS_S) {                                     // the per-sample scale of tsr_ssim_fwd_bwd_ps
    const float sb = scale[blockIdx.x];
    if (sb == 0.f) {                                         // skipped: no window work, nothing of the image is read
      ssim_skip<HAS_DY>(ssim, dy, n, accumulate);
      return;
    }
    dy_scale *= (double)sb;
  }
  const float* py = y + (size_t)blockIdx.x * n;
  const float* pt = t + (size_t)blockIdx.x * n;
  double s[5] = {0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < n; i += SSIM_THREADS) {
    const double a = py[i], b = pt[i];
    s[0] += a; s[1] += b; s[2] += a * a; s[3] += b * b; s[4] += a * b;
  }
  for (int k = 0; k < 5; ++k) sh[threadIdx.x * 5 + k] = s[k];
  __syncthreads();
  for (int st = SSIM_THREADS / 2; st > 0; st >>= 1) {
    if (threadIdx.x < st)
      for (int k = 0; k < 5; ++k) sh[threadIdx.x * 5 + k] += sh[(threadIdx.x + st) * 5 + k];
    __syncthreads();
  }
  const double mx = sh[0] / n, mt = sh[1] / n;
  const double sxx = sh[2] / n - mx * mx, stt = sh[3] / n - mt * mt, sxt = sh[4] / n - mx * mt;
  const double A1 = 2 * mx * mt + C1, A2 = 2 * sxt + C2, B1 = mx * mx + mt * mt + C1, B2 = sxx + stt + C2;
  const double S = (A1 * A2) / (B1 * B2);
  if (threadIdx.x == 0) ssim[blockIdx.x] = (float)S;
  if constexpr (HAS_DY) {
    const double inv = 1.0 / (B1 * B2);
    const double coef = dy_scale / n;
    const double P = coef * (2 * mt * (A2 - A1) * inv - 2 * mx * S * (1.0 / B1 - 1.0 / B2));
    const double Q = coef * 2 * (-S / B2), R = coef * (2 * A1 * inv);
    float* pd = dy + (size_t)blockIdx.x * n;
    for (int i = threadIdx.x; i < n; i += SSIM_THREADS) {
      const double v = P + (double)py[i] * Q + (double)pt[i] * R;
      pd[i] = accumulate ? (float)((double)pd[i] + v) : (float)v;
    }
  }
}

// ------------------------------------------------------------------------------------------
// Windowed form.  The workgroup walks its image in steps of `rows` rows.  A step
//   1. loads the rows + WIN - 1 input rows its new map rows read                          (sX, sT: fp32)
//   2. vertical pass: the five moments' column sums for the new map rows                   (sV[5][rows][W])
//   3. horizontal pass: the moments, S (into the thread's running sum) and P, Q, R into a ring of the last
//      rows + WIN - 1 map rows                                                             (sRing[3][ring][Wo])
//   4. vertical adjoint of the ring for the step's dy rows (row r reads map rows r-WIN+1..r) (sD = sV, [3][rows][Wo])
//   5. horizontal adjoint, the combination with x_p and t_p, and the store.
// The ring is what spares a 2 (WIN - 1) row halo: no map row is computed twice.  HAS_DY = false stops after step 3 and
// keeps no ring.
// ------------------------------------------------------------------------------------------
template <int WIN, bool HAS_DY, bool HAS_S>
__global__ __launch_bounds__(SSIM_THREADS) void ssim_win_kernel(const float* __restrict__ y,
                                                                const float* __restrict__ t, int H, int W, int rows,
                                                                ssim_gauss gw, double C1, double C2,
                                                                float* __restrict__ ssim, float* __restrict__ dy,
                                                                double dy_scale, int accumulate,
                                                                const float* __restrict__ s) {
  extern __shared__ double ssim_smem[];
  __shared__ double sred[SSIM_THREADS];
  if constexpr (HAS_S) {
    const float sb = s[blockIdx.x];
    if (sb == 0.f) {
      ssim_skip<HAS_DY>(ssim, dy, H * W, accumulate);
      return;
    }
    dy_scale *= (double)sb;
  }
  constexpr int PAD = WIN - 1;
  const int Ho = H - PAD, Wo = W - PAD, ring = rows + PAD;
  double* sV = ssim_smem;                                              // [5][rows][W]; sD [3][rows][Wo] aliases it
  double* sRing = sV + 5 * rows * W;                                   // [3][ring][Wo]
  float* sX = (float*)(sRing + (HAS_DY ? 3 * ring * Wo : 0));          // [rows + PAD][W]
  float* sT = sX + (rows + PAD) * W;
  const float* py = y + (size_t)blockIdx.x * H * W;
  const float* pt = t + (size_t)blockIdx.x * H * W;
  float* pd = HAS_DY ? dy + (size_t)blockIdx.x * H * W : nullptr;
  const int tid = threadIdx.x;
  const double coef = dy_scale / ((double)Ho * (double)Wo);
  double ssum = 0;

  const int r_end = HAS_DY ? H : Ho;
  for (int r0 = 0; r0 < r_end; r0 += rows) {
    const int n_new = min(r0 + rows, Ho) - r0;                         // new map rows r0 .. r0 + n_new - 1 (<= 0: none left)
    if (n_new > 0) {
      const int n_in = (n_new + PAD) * W;                              // r0 + n_new + PAD <= H
      for (int i = tid; i < n_in; i += SSIM_THREADS) {
        sX[i] = py[r0 * W + i];
        sT[i] = pt[r0 * W + i];
      }
      __syncthreads();
      for (int it = tid; it < n_new * W; it += SSIM_THREADS) {
        const int mi = it / W, c = it - mi * W;
        double a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0;
#pragma unroll
        for (int i = 0; i < WIN; ++i) {
          const double xv = sX[(mi + i) * W + c], tv = sT[(mi + i) * W + c];
          const double gx = gw.g[i] * xv, gt = gw.g[i] * tv;
          a0 += gx; a1 += gt;
          a2 = fma(gx, xv, a2); a3 = fma(gt, tv, a3); a4 = fma(gx, tv, a4);
        }
        sV[(0 * rows + mi) * W + c] = a0; sV[(1 * rows + mi) * W + c] = a1; sV[(2 * rows + mi) * W + c] = a2;
        sV[(3 * rows + mi) * W + c] = a3; sV[(4 * rows + mi) * W + c] = a4;
      }
      __syncthreads();
      for (int it = tid; it < n_new * Wo; it += SSIM_THREADS) {
        const int mi = it / Wo, j = it - mi * Wo;
        double m[5] = {0, 0, 0, 0, 0};
#pragma unroll
        for (int jj = 0; jj < WIN; ++jj) {
#pragma unroll
          for (int k = 0; k < 5; ++k) m[k] = fma(gw.g[jj], sV[(k * rows + mi) * W + j + jj], m[k]);
        }
        const double mx = m[0], mt = m[1];
        const double sxx = m[2] - mx * mx, stt = m[3] - mt * mt, sxt = m[4] - mx * mt;
        const double A1 = 2 * mx * mt + C1, A2 = 2 * sxt + C2, B1 = mx * mx + mt * mt + C1, B2 = sxx + stt + C2;
        const double S = (A1 * A2) / (B1 * B2);
        ssum += S;
        if constexpr (HAS_DY) {
          const double inv = 1.0 / (B1 * B2);
          const int slot = (r0 + mi) % ring;
          sRing[(0 * ring + slot) * Wo + j] = 2 * mt * (A2 - A1) * inv - 2 * mx * S * (1.0 / B1 - 1.0 / B2);
          sRing[(1 * ring + slot) * Wo + j] = -S / B2;
          sRing[(2 * ring + slot) * Wo + j] = 2 * A1 * inv;
        }
      }
    }
    if constexpr (HAS_DY) {
      __syncthreads();                                                 // sV is read, the ring written: sD may overwrite sV
      const int n_out = min(rows, H - r0);                             // dy rows r0 .. r0 + n_out - 1
      double* sD = sV;
      for (int it = tid; it < n_out * Wo; it += SSIM_THREADS) {
        const int ri = it / Wo, j = it - ri * Wo, r = r0 + ri;
        double d0 = 0, d1 = 0, d2 = 0;
#pragma unroll
        for (int i = 0; i < WIN; ++i) {
          const int mrow = r - i;                                      // in [r0 - PAD, r0 + rows): inside the ring
          if (mrow >= 0 && mrow < Ho) {
            const int slot = mrow % ring;
            d0 = fma(gw.g[i], sRing[(0 * ring + slot) * Wo + j], d0);
            d1 = fma(gw.g[i], sRing[(1 * ring + slot) * Wo + j], d1);
            d2 = fma(gw.g[i], sRing[(2 * ring + slot) * Wo + j], d2);
          }
        }
        sD[(0 * rows + ri) * Wo + j] = d0; sD[(1 * rows + ri) * Wo + j] = d1; sD[(2 * rows + ri) * Wo + j] = d2;
      }
      __syncthreads();
      for (int it = tid; it < n_out * W; it += SSIM_THREADS) {
        const int ri = it / W, c = it - ri * W;
        double u0 = 0, u1 = 0, u2 = 0;
#pragma unroll
        for (int jj = 0; jj < WIN; ++jj) {
          const int j = c - jj;
          if (j >= 0 && j < Wo) {
            u0 = fma(gw.g[jj], sD[(0 * rows + ri) * Wo + j], u0);
            u1 = fma(gw.g[jj], sD[(1 * rows + ri) * Wo + j], u1);
            u2 = fma(gw.g[jj], sD[(2 * rows + ri) * Wo + j], u2);
          }
        }
        const int idx = (r0 + ri) * W + c;
        const double v = coef * (u0 + 2.0 * (double)py[idx] * u1 + (double)pt[idx] * u2);
        pd[idx] = accumulate ? (float)((double)pd[idx] + v) : (float)v;
      }
      // the next step's load barrier orders these sD reads before its sV writes
    }
  }
  const double total = ssim_block_sum(ssum, sred);
  if (tid == 0) ssim[blockIdx.x] = (float)(total / ((double)Ho * (double)Wo));
}

// Dynamic LDS of a step of `rows` rows.
size_t ssim_win_smem(int rows, int W, int win, bool has_dy) {
  const int pad = win - 1, Wo = W - pad;
  return sizeof(double) * ((size_t)5 * rows * W + (has_dy ? (size_t)3 * (rows + pad) * Wo : 0)) +
         sizeof(float) * (size_t)2 * (rows + pad) * W;
}

constexpr size_t SSIM_SMEM_SMALL = 60 * 1024;     // needs no attribute and leaves room for a second workgroup per CU
constexpr size_t SSIM_SMEM_LARGE = 152 * 1024;    // with the 2 KB static buffer, inside the 160 KB of a CU
constexpr int SSIM_MAX_ROWS = 16;

// Rows per step: a function of the shape only (the same shape always takes the same summation order).  The largest
// step of at most 16 rows that fits the small budget; wide images, where that would be under 8 rows, take the large one.
int ssim_win_rows(int H, int W, int win, bool has_dy, size_t* smem) {
  const int top = H < SSIM_MAX_ROWS ? H : SSIM_MAX_ROWS;
  int rows = top;
  while (rows > 1 && ssim_win_smem(rows, W, win, has_dy) > SSIM_SMEM_SMALL) --rows;
  if (rows < (top < 8 ? top : 8) || ssim_win_smem(rows, W, win, has_dy) > SSIM_SMEM_SMALL) {
    rows = top;
    while (rows > 1 && ssim_win_smem(rows, W, win, has_dy) > SSIM_SMEM_LARGE) --rows;
  }
  *smem = ssim_win_smem(rows, W, win, has_dy);
  return rows;
}

template <int WIN, bool HAS_DY, bool HAS_S>
int ssim_win_launch(const float* y, const float* t, int B, int H, int W, const ssim_gauss& gw, double C1, double C2,
                    float* ssim, float* dy, double dy_scale, int accumulate, const float* s, hipStream_t st) {
  size_t smem = 0;
  const int rows = ssim_win_rows(H, W, WIN, HAS_DY, &smem);
  if (smem > SSIM_SMEM_LARGE) return TSR_ERR_ARG;
  if (smem > 64 * 1024) {
    static bool attr_set = false;
    if (!attr_set) {
      (void)hipFuncSetAttribute((const void*)ssim_win_kernel<WIN, HAS_DY, HAS_S>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)SSIM_SMEM_LARGE);
      attr_set = true;
    }
  }
  hipLaunchKernelGGL((ssim_win_kernel<WIN, HAS_DY, HAS_S>), dim3(B), dim3(SSIM_THREADS), smem, st, y, t, H, W, rows, gw, C1, C2,
                     ssim, dy, dy_scale, accumulate, s);
  return tsr_check_launch();
}

template <int WIN>
int ssim_win_dispatch(const float* y, const float* t, int B, int H, int W, const ssim_gauss& gw, double C1, double C2,
                      float* ssim, float* dy, double dy_scale, int accumulate, const float* s, hipStream_t st) {
  if (s)      // the unscaled instantiations are the kernels as they were before the scale existed
    return dy ? ssim_win_launch<WIN, true, true>(y, t, B, H, W, gw, C1, C2, ssim, dy, dy_scale, accumulate, s, st)
              : ssim_win_launch<WIN, false, true>(y, t, B, H, W, gw, C1, C2, ssim, dy, dy_scale, accumulate, s, st);
  return dy ? ssim_win_launch<WIN, true, false>(y, t, B, H, W, gw, C1, C2, ssim, dy, dy_scale, accumulate, s, st)
            : ssim_win_launch<WIN, false, false>(y, t, B, H, W, gw, C1, C2, ssim, dy, dy_scale, accumulate, s, st);
}

// tsr_ssim_fwd_bwd (s NULL) and tsr_ssim_fwd_bwd_ps: one argument check, one launch.
int ssim_entry(const float* y, const float* t, int B, int H, int W, int win, double sigma, double C1, double C2,
               float* ssim, float* dy, float dy_scale, int accumulate, const float* s, void* stream) {
  if (!y || !t || !ssim || B <= 0 || H <= 0 || W <= 0) return TSR_ERR_ARG;
  if (!(C1 > 0) || !(C2 > 0) || dy_scale != dy_scale) return TSR_ERR_ARG;          // !(c > 0) catches NaN
  if (accumulate != 0 && accumulate != 1) return TSR_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (win == 0) {
    if ((long long)H * W > (1LL << 28)) return TSR_ERR_ARG;
    const int n = H * W;
    const dim3 grid(B), block(SSIM_THREADS);
    const double sc = (double)dy_scale;
    if (dy && s)
      hipLaunchKernelGGL((ssim_global_kernel<true, true>), grid, block, 0, st, y, t, n, C1, C2, ssim, dy, sc, accumulate, s);
    else if (dy)
      hipLaunchKernelGGL((ssim_global_kernel<true, false>), grid, block, 0, st, y, t, n, C1, C2, ssim, dy, sc, accumulate, s);
    else if (s)
      hipLaunchKernelGGL((ssim_global_kernel<false, true>), grid, block, 0, st, y, t, n, C1, C2, ssim, dy, sc, accumulate, s);
    else
      hipLaunchKernelGGL((ssim_global_kernel<false, false>), grid, block, 0, st, y, t, n, C1, C2, ssim, dy, sc, accumulate, s);
    return tsr_check_launch();
  }
  if (win < 3 || win > SSIM_MAX_WIN || !(win & 1)) return TSR_ERR_ARG;
  if (H < win || W < win || H > SSIM_MAX_HW || W > SSIM_MAX_HW) return TSR_ERR_ARG;
  if (!(sigma > 0)) return TSR_ERR_ARG;
  ssim_gauss gw;
  double sum = 0;
  for (int k = 0; k < SSIM_MAX_WIN; ++k) {
    const double d = k - 0.5 * (win - 1);
    gw.g[k] = k < win ? exp(-d * d / (2.0 * sigma * sigma)) : 0.0;
    sum += gw.g[k];
  }
  if (!(sum > 0)) return TSR_ERR_ARG;                       // a sigma whose square underflows: the centre tap is 0/0
  for (int k = 0; k < win; ++k) gw.g[k] /= sum;
  const double sc = (double)dy_scale;
  switch (win) {
    case 3: return ssim_win_dispatch<3>(y, t, B, H, W, gw, C1, C2, ssim, dy, sc, accumulate, s, st);
    case 5: return ssim_win_dispatch<5>(y, t, B, H, W, gw, C1, C2, ssim, dy, sc, accumulate, s, st);
    case 7: return ssim_win_dispatch<7>(y, t, B, H, W, gw, C1, C2, ssim, dy, sc, accumulate, s, st);
    case 9: return ssim_win_dispatch<9>(y, t, B, H, W, gw, C1, C2, ssim, dy, sc, accumulate, s, st);
    default: return ssim_win_dispatch<11>(y, t, B, H, W, gw, C1, C2, ssim, dy, sc, accumulate, s, st);
  }
}

}  // namespace

extern "C" int tsr_ssim_fwd_bwd(const float* y, const float* t, int B, int H, int W, int win, double sigma, double C1,
                                double C2, float* ssim, float* dy, float dy_scale, int accumulate, void* stream) {
  return ssim_entry(y, t, B, H, W, win, sigma, C1, C2, ssim, dy, dy_scale, accumulate, nullptr, stream);
}

extern "C" int tsr_ssim_fwd_bwd_ps(const float* y, const float* t, int B, int H, int W, int win, double sigma, double C1,
                                   double C2, const float* s, float* ssim, float* dy, float dy_scale, int accumulate,
                                   void* stream) {
  return ssim_entry(y, t, B, H, W, win, sigma, C1, C2, ssim, dy, dy_scale, accumulate, s, stream);
}
