// Contact readout: the geometry of the contact region of a pressure image -- pixel count, area, mass, peak, centroid,
// second moments, orientation and axes -- and, for a pair (output, target), the overlap and error metrics between the
// two regions, from one launch (tsr_contact_readout, include/tactilesr_hip.h, where every formula is written out).
//
//   tau   = (double)(float)threshold                      (mode 0)     mn + threshold (mx - mn)      (mode 1, no contraction)
//   m_p   = [(double)v_p > tau]
//   u(x)  = (x + 0.5) span_r / H - 0.5,  v(c) = (c + 0.5) span_c / W - 0.5
//
// Everything is fp64 from the exact fp32 pixels; a value is rounded to fp32 once, at its store.
//
// One workgroup of 256 threads owns one image (one pair) and walks the batch at a stride of the grid.  Thread k owns the
// quads j = k, k + 256, ... of the flat image: pixels 4j .. 4j+3, so consecutive threads read consecutive 16 bytes.
//   pass 1:  min, max, the first maximum in row-major order and a non-finite flag; a wave64 by shuffles, the four waves
//            through LDS.  (max, index) pairs combine to the larger value and on ties the smaller index: no order matters.
//   pass 2:  re-reads the image (from cache) and sums, per image, sum v and -- over the mask -- v, v dx, v dc, v dx^2,
//            v dc^2, v dx dc with (dx, dc) the INTEGER pixel offset from the peak, and the mask counts.  v (24 bits) times an
//            offset (< 2^24) is exact in fp64 and the offsets are small near the contact: a one-pixel contact has exactly
//            zero moments, and mu = sum/M - mean^2 does not cancel the image's distance from the origin.  The counts are
//            integers; the sums are reduced in a fixed order (shuffle tree, then waves 0..3).
//   finish:  thread 0 turns the sums of y into its record, thread 64 those of t, thread 0 then writes the pair.
// The quad map and the order depend on (H, W) alone.  16-byte loads when W % 4 == 0 and the image base is 16-byte
// aligned; otherwise the same four pixels are loaded one float at a time and go through the same instructions.  No
// atomics and nothing read back: two launches, and launches under different grid caps, give the same bits.
#include <math.h>

#include "tsr_common.h"
#include "tactilesr_hip.h"

namespace {

constexpr int CR_THREADS = 256;
constexpr int CR_WAVES = CR_THREADS / 64;
constexpr int CR_NSUM = 7;                    // sum v; over the mask: v, v dx, v dc, v dx^2, v dc^2, v dx dc
constexpr int CR_FIN = 8;                     // cu, cv, M, theta, peak u, peak v, n, bad

struct cr_args {
  const float* img[2];                        // y, t
  float* rec[2];
  float* pair;
  double threshold, gain, span_r, span_c;
  int B, H, W, mode;
  int vec[2];
};

__device__ __forceinline__ void cr_load4(const float* img, unsigned i0, int nv, int vec, float f[4]) {
  if (vec) {
    const float4 q = *reinterpret_cast<const float4*>(img + i0);
    f[0] = q.x; f[1] = q.y; f[2] = q.z; f[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = j < nv ? img[i0 + j] : 0.f;
  }
}

// mn + threshold (mx - mn) as a separate subtraction, product and sum: a numpy restatement reproduces the bits.
__device__ __forceinline__ double cr_tau_range(double mn, double mx, double threshold) {
#pragma clang fp contract(off)
  const double d = mx - mn;
  const double m = threshold * d;
  return mn + m;
}

// The record of one image from its reduced sums; `fin` receives what the pair needs.  Not inlined and not contracted: the
// single and the pair kernel run the same instructions, so a record does not depend on the form it was asked in.
__device__ __noinline__ void cr_finish(const cr_args& p, const double* s, unsigned n, float mxf, unsigned idx, unsigned bad,
                                       double tau, float* rec, double* fin) {
#pragma clang fp contract(off)
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  const double H = (double)p.H, W = (double)p.W;
  const double pr = p.span_r / H, pc = p.span_c / W;
  const unsigned xpk = idx / (unsigned)p.W, cpk = idx - xpk * (unsigned)p.W;
  const double upk = ((double)xpk + 0.5) * p.span_r / H - 0.5, vpk = ((double)cpk + 0.5) * p.span_c / W - 0.5;
  double o[TSR_CONTACT_REC];
  o[0] = (double)n;
  o[1] = (double)n * pr * pc;
  o[2] = p.gain * s[1];
  o[3] = p.gain * s[0];
  o[4] = p.gain * (double)mxf;
  o[5] = upk;
  o[6] = vpk;
  o[15] = tau;
  if (n == 0 || !(s[1] > 0.0)) {
#pragma unroll
    for (int i = 7; i < 15; ++i) o[i] = qnan;
  } else {
    const double inv = 1.0 / s[1];
    const double ex = s[2] * inv, ec = s[3] * inv;                // the mean offset from the peak, in pixels
    const double muu = pr * pr * (s[4] * inv - ex * ex), mvv = pc * pc * (s[5] * inv - ec * ec);
    const double muv = pr * pc * (s[6] * inv - ex * ec);
    o[7] = upk + pr * ex;
    o[8] = vpk + pc * ec;
    o[9] = muu; o[10] = mvv; o[11] = muv;
    const double a2 = 2.0 * muv, a1 = muu - mvv;
    double th = (a2 == 0.0 && a1 == 0.0) ? 0.0 : 0.5 * atan2(a2, a1);
    if ((float)th <= -(float)M_PI_2) th = M_PI_2;                 // the same axis: the stored fp32 stays in (-pi/2, pi/2]
    o[12] = th;
    const double h = 0.5 * (muu + mvv), d = sqrt(0.25 * a1 * a1 + muv * muv);
    const double lp = h + d, lm = h - d;
    o[13] = sqrt(lp > 0.0 ? lp : 0.0);
    o[14] = sqrt(lm > 0.0 ? lm : 0.0);
  }
  if (bad) {
#pragma unroll
    for (int i = 0; i < TSR_CONTACT_REC; ++i) o[i] = qnan;
  }
  if (rec) {
#pragma unroll
    for (int i = 0; i < TSR_CONTACT_REC; ++i) rec[i] = (float)o[i];
  }
  fin[0] = o[7]; fin[1] = o[8]; fin[2] = o[2]; fin[3] = o[12]; fin[4] = o[5]; fin[5] = o[6];
  fin[6] = (double)n; fin[7] = bad ? 1.0 : 0.0;
}

template <bool PAIR>
__global__ __launch_bounds__(CR_THREADS) void contact_kernel(cr_args p) {
#pragma clang fp contract(off)                                    // the sums below name their fmas: both forms, the same bits
  constexpr int NI = PAIR ? 2 : 1;
  __shared__ float sMn[NI][CR_WAVES], sMx[NI][CR_WAVES];
  __shared__ unsigned sIdx[NI][CR_WAVES], sBad[NI][CR_WAVES];
  __shared__ double sPart[CR_WAVES][NI * CR_NSUM];
  __shared__ unsigned sCnt[CR_WAVES][3];
  __shared__ double sTot[NI * CR_NSUM];
  __shared__ double sFin[NI][CR_FIN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned W = (unsigned)p.W, P = (unsigned)p.H * (unsigned)p.W, nq = (P + 3u) >> 2;

  for (int b = blockIdx.x; b < p.B; b += gridDim.x) {
    __syncthreads();                                              // the previous image's reads of the shared arrays
    const float* img[NI];
#pragma unroll
    for (int k = 0; k < NI; ++k) img[k] = p.img[k] + (size_t)b * P;

    // ---- pass 1: min, max, first argmax, non-finite flag
    float mn[NI], mx[NI];
    unsigned idx[NI], bad[NI];
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      mn[k] = __int_as_float(0x7f800000); mx[k] = __int_as_float(0xff800000); idx[k] = 0xffffffffu; bad[k] = 0u;
    }
    for (unsigned q = tid; q < nq; q += CR_THREADS) {
      const unsigned i0 = 4u * q;
      const int nv = (int)min(4u, P - i0);
#pragma unroll
      for (int k = 0; k < NI; ++k) {
        float f[4];
        cr_load4(img[k], i0, nv, p.vec[k], f);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j < nv) {
            const float v = f[j];
            bad[k] |= ((__float_as_uint(v) & 0x7f800000u) == 0x7f800000u) ? 1u : 0u;
            if (v < mn[k]) mn[k] = v;
            if (v > mx[k]) { mx[k] = v; idx[k] = i0 + j; }        // strict: the first maximum of the thread's pixels
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < NI; ++k) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const float omn = __shfl_down(mn[k], off, 64), omx = __shfl_down(mx[k], off, 64);
        const unsigned oidx = __shfl_down(idx[k], off, 64), obad = __shfl_down(bad[k], off, 64);
        if (omn < mn[k]) mn[k] = omn;
        if (omx > mx[k] || (omx == mx[k] && oidx < idx[k])) { mx[k] = omx; idx[k] = oidx; }
        bad[k] |= obad;
      }
      if (lane == 0) { sMn[k][wave] = mn[k]; sMx[k][wave] = mx[k]; sIdx[k][wave] = idx[k]; sBad[k][wave] = bad[k]; }
    }
    __syncthreads();
    double tau[NI];
    int xpk[NI], cpk[NI];
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      mn[k] = sMn[k][0]; mx[k] = sMx[k][0]; idx[k] = sIdx[k][0]; bad[k] = sBad[k][0];
#pragma unroll
      for (int w = 1; w < CR_WAVES; ++w) {
        const float omn = sMn[k][w], omx = sMx[k][w];
        const unsigned oidx = sIdx[k][w];
        if (omn < mn[k]) mn[k] = omn;
        if (omx > mx[k] || (omx == mx[k] && oidx < idx[k])) { mx[k] = omx; idx[k] = oidx; }
        bad[k] |= sBad[k][w];
      }
      tau[k] = p.mode == 0 ? (double)(float)p.threshold : cr_tau_range((double)mn[k], (double)mx[k], p.threshold);
      const unsigned xp = idx[k] / W;
      xpk[k] = (int)xp; cpk[k] = (int)(idx[k] - xp * W);
    }

    // ---- pass 2: counts and moments about the peak pixel
    double acc[NI][CR_NSUM];
    unsigned cnt[3] = {0u, 0u, 0u};                               // n_y, n_t, intersection
#pragma unroll
    for (int k = 0; k < NI; ++k)
#pragma unroll
      for (int i = 0; i < CR_NSUM; ++i) acc[k][i] = 0.0;
    for (unsigned q = tid; q < nq; q += CR_THREADS) {
      const unsigned i0 = 4u * q;
      const int nv = (int)min(4u, P - i0);
      float f[NI][4];
#pragma unroll
      for (int k = 0; k < NI; ++k) cr_load4(img[k], i0, nv, p.vec[k], f[k]);
      unsigned x = i0 / W, c = i0 - x * W;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (c >= W) { c -= W; ++x; }
        if (j < nv) {
          bool both = true;
#pragma unroll
          for (int k = 0; k < NI; ++k) {
            const double v = (double)f[k][j];
            const bool m = v > tau[k];
            const double w = m ? v : 0.0;
            const double dx = (double)((int)x - xpk[k]), dc = (double)((int)c - cpk[k]);
            const double wx = w * dx, wc = w * dc;                   // exact: 24 bits times an integer below 2^24
            acc[k][0] += v;
            acc[k][1] += w;
            acc[k][2] += wx;
            acc[k][3] += wc;
            acc[k][4] = fma(wx, dx, acc[k][4]);
            acc[k][5] = fma(wc, dc, acc[k][5]);
            acc[k][6] = fma(wx, dc, acc[k][6]);
            cnt[k] += m ? 1u : 0u;
            both = both && m;
          }
          if (PAIR) cnt[2] += both ? 1u : 0u;
        }
        ++c;
      }
    }
#pragma unroll
    for (int k = 0; k < NI; ++k)
#pragma unroll
      for (int i = 0; i < CR_NSUM; ++i) {
        double v = acc[k][i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) sPart[wave][k * CR_NSUM + i] = v;
      }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      unsigned v = cnt[i];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
      if (lane == 0) sCnt[wave][i] = v;
    }
    __syncthreads();
    if (tid < NI * CR_NSUM) {
      double s = sPart[0][tid];
      for (int w = 1; w < CR_WAVES; ++w) s += sPart[w][tid];
      sTot[tid] = s;
    }
    __syncthreads();

    // ---- finish: one thread an image, then the pair
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      if (tid == 64 * k) {
        unsigned n = 0;
        for (int w = 0; w < CR_WAVES; ++w) n += sCnt[w][k];
        cr_finish(p, sTot + k * CR_NSUM, n, mx[k], idx[k], bad[k], tau[k],
                  p.rec[k] ? p.rec[k] + (size_t)b * TSR_CONTACT_REC : nullptr, sFin[k]);
      }
    }
    if (PAIR) {
      __syncthreads();
      if (tid == 0) {
        const double qnan = __longlong_as_double(0x7ff8000000000000LL);
        const double* fy = sFin[0];
        const double* ft = sFin[1];
        unsigned ni = 0;
        for (int w = 0; w < CR_WAVES; ++w) ni += sCnt[w][2];
        const double ny = fy[6], nt = ft[6], inter = (double)ni, uni = ny + nt - inter;
        double o[TSR_CONTACT_PAIR];
        o[0] = inter;
        o[1] = uni;
        o[2] = uni > 0.0 ? inter / uni : 1.0;
        o[3] = ny + nt > 0.0 ? 2.0 * inter / (ny + nt) : 1.0;
        const double du = fy[0] - ft[0], dv = fy[1] - ft[1];      // NaN when either contact has no centroid
        o[4] = sqrt(du * du + dv * dv);
        o[5] = (nt > 0.0 && ft[2] > 0.0) ? fabs(fy[2] - ft[2]) / ft[2] : qnan;
        const double pu = fy[4] - ft[4], pv = fy[5] - ft[5];
        o[6] = sqrt(pu * pu + pv * pv);
        double dth = fabs(fy[3] - ft[3]);                         // both in (-pi/2, pi/2]: the difference is in [0, pi)
        if (dth > M_PI_2) dth = M_PI - dth;
        o[7] = dth;
        const bool nanall = fy[7] != 0.0 || ft[7] != 0.0;
        float* dst = p.pair + (size_t)b * TSR_CONTACT_PAIR;
#pragma unroll
        for (int i = 0; i < TSR_CONTACT_PAIR; ++i) dst[i] = (float)(nanall ? qnan : o[i]);
      }
    }
  }
}

inline bool cr_finite(double v) { return v >= -1.79769313486231570e308 && v <= 1.79769313486231570e308; }

inline bool cr_overlap(const void* a, size_t na, const void* b, size_t nb) {          // sizes in floats; NULL overlaps nothing
  if (!a || !b) return false;
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + 4 * nb && pb < pa + 4 * na;
}

}  // namespace

extern "C" int tsr_contact_readout_wgs(const float* y, const float* t, int B, int H, int W, int mode, double threshold,
                                       double gain, double span_r, double span_c, float* rec_y, float* rec_t, float* pair,
                                       int max_wgs, void* stream) {
  if (!y || !rec_y || B <= 0 || H <= 0 || W <= 0) return TSR_ERR_ARG;
  if ((long long)H * (long long)W > (1LL << 24)) return TSR_ERR_ARG;
  if (mode != 0 && mode != 1) return TSR_ERR_ARG;
  if (!cr_finite(threshold) || !cr_finite(gain)) return TSR_ERR_ARG;
  if (mode == 1 && !(threshold >= 0.0 && threshold < 1.0)) return TSR_ERR_ARG;
  if (!cr_finite(span_r) || !cr_finite(span_c) || !(span_r > 0.0) || !(span_c > 0.0)) return TSR_ERR_ARG;
  if (!t && (rec_t || pair)) return TSR_ERR_ARG;
  if (t && !pair) return TSR_ERR_ARG;
  if (max_wgs < 1) return TSR_ERR_ARG;
  const size_t n = (size_t)B * H * W, nr = (size_t)B * TSR_CONTACT_REC, np = (size_t)B * TSR_CONTACT_PAIR;
  const void* ins[2] = {y, t};
  const void* outs[3] = {rec_y, rec_t, pair};
  const size_t nouts[3] = {nr, nr, np};
  for (int o = 0; o < 3; ++o) {
    for (int i = 0; i < 2; ++i)
      if (cr_overlap(outs[o], nouts[o], ins[i], n)) return TSR_ERR_ARG;
    for (int o2 = o + 1; o2 < 3; ++o2)
      if (cr_overlap(outs[o], nouts[o], outs[o2], nouts[o2])) return TSR_ERR_ARG;
  }
  cr_args p;
  p.img[0] = y; p.img[1] = t; p.rec[0] = rec_y; p.rec[1] = rec_t; p.pair = pair;
  p.threshold = threshold; p.gain = gain; p.span_r = span_r; p.span_c = span_c;
  p.B = B; p.H = H; p.W = W; p.mode = mode;
  p.vec[0] = (W % 4 == 0) && ((uintptr_t)y & 15) == 0;
  p.vec[1] = t && (W % 4 == 0) && ((uintptr_t)t & 15) == 0;
  const int wgs = B < max_wgs ? B : max_wgs;
  if (t)
    hipLaunchKernelGGL(contact_kernel<true>, dim3(wgs), dim3(CR_THREADS), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(contact_kernel<false>, dim3(wgs), dim3(CR_THREADS), 0, (hipStream_t)stream, p);
  return tsr_check_launch();
}

extern "C" int tsr_contact_readout(const float* y, const float* t, int B, int H, int W, int mode, double threshold,
                                   double gain, double span_r, double span_c, float* rec_y, float* rec_t, float* pair,
                                   void* stream) {
  return tsr_contact_readout_wgs(y, t, B, H, W, mode, threshold, gain, span_r, span_c, rec_y, rec_t, pair,
                                 TSR_CONTACT_MAX_WGS, stream);
}
