// Taxel sensor-noise augmentation on the device: per-taxel gain drift, heteroscedastic Gaussian read-out noise and dead
// taxels in ONE launch, driven by a counter-based generator (tsr_taxel_noise, include/tactilesr_hip.h).
//
// Generator: Philox4x32-10, key (seed_lo, seed_hi), counter (block, id, offset, tag).  One block gives four words
// r0..r3; lane l of block j serves item 4 j + l of the effect `tag` (0 noise, 1 gain, 2 dropout) of sample `id`.
// For element i = c P + p of a sample (P = H W, axis = c % axis_cnt), in this order:
//   gain     item axis P + p:  u = (r >> 8) 2^-24,  g = fmaf(gain_jitter, 2 u - 1, 1),  v = g x          (one rounding each)
//   noise    item i; words (r0, r1) give items 4 j, 4 j + 1 and (r2, r3) items 4 j + 2, 4 j + 3:
//            u1 = (2 (ra >> 9) + 1) 2^-24,  u2 = (rb >> 8) 2^-24,  R = sqrtf(-2 logf(u1)),
//            n_a = R cospif(2 u2),  n_b = R sinpif(2 u2)                                       (products rounded once)
//            t = sigma_mul[axis] v,  s = sqrtf(fmaf(t, t, sigma_add[axis]^2)),  y = fmaf(s, n, v)
//   dropout  item p:  dead when (r >> 8) < drop_thresh; a dead taxel reads drop_value (a select: it replaces a NaN too)
// A neutral effect (gain_jitter == 0; both sigmas of the axis 0; drop_thresh == 0) is skipped, not computed with zeros:
// data move as 32-bit patterns until an effect touches them, so with everything neutral out == x bit for bit.
//
// Shape: memory-trivial (11 MB at B = 8192 for the Seqs taxels), so one thread per four consecutive elements of a sample
// (work item (b, j): elements 4 j .. 4 j + 3 of sample b, the noise block j), a grid-stride walk under the caller's cap,
// 16-byte loads and stores when P % 4 == 0 and both bases are 16-byte aligned (then the four elements share a channel,
// one gain block and one dropout block), single dwords otherwise.  Both forms run the same per-element code, and every
// fp32 operation is spelled with its rounding (no contraction left to the compiler): the bits do not depend on the
// path, the grid or the batch.  A thread reads its elements before it writes them, and nobody else touches them: out may
// be x itself.  Plain vector stores only; no atomics, no LDS.
#include "tsr_common.h"
#include "tactilesr_hip.h"

#include <math.h>
#include <string.h>

namespace {

constexpr int TN_THREADS = 256;                     // four wave64
constexpr int TN_MAX_WGS = 1 << 20;                 // tsr_taxel_noise's grid cap (TSR_TAXEL_NOISE_MAX_WGS)
constexpr unsigned TN_NAN = 0x7fc00000u;
constexpr unsigned TN_M0 = 0xD2511F53u, TN_M1 = 0xCD9E8D57u;
constexpr unsigned TN_W0 = 0x9E3779B9u, TN_W1 = 0xBB67AE85u;
constexpr float TN_2M24 = 5.9604644775390625e-08f;  // 2^-24

struct tn_params {
  const unsigned* x;
  unsigned* out;
  const long long* ids;
  const unsigned* rng;                              // device {seed_lo, seed_hi, offset, 0}, or NULL: the three below
  long long id_base;
  long long B;
  int P, CHW, nb;                                   // nb = ceil(CHW / 4) work items a sample
  int axis_cnt;
  unsigned seed_lo, seed_hi, offset;
  unsigned drop_thresh, drop_bits;
  int noise_mask;                                   // bit a: axis a has a non-zero sigma
  float gain_jitter;
  float sigma_add[4], sigma_mul[4];
};

__device__ __forceinline__ uint4 tn_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned h0 = __umulhi(TN_M0, c0), l0 = TN_M0 * c0;
    const unsigned h1 = __umulhi(TN_M1, c2), l1 = TN_M1 * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += TN_W0;
    k1 += TN_W1;
  }
  return make_uint4(c0, c1, c2, c3);
}

__device__ __forceinline__ unsigned tn_lane(const uint4& w, unsigned l) {
  return l == 0 ? w.x : (l == 1 ? w.y : (l == 2 ? w.z : w.w));
}

// The stream of one (sample, effect): the block of the last item asked for is kept, so the four elements of a thread
// that share a block (always on the 16-byte path) pay for one Philox call.
struct tn_stream {
  unsigned id, offset, tag, k0, k1;
  unsigned blk;
  uint4 w;
  __device__ __forceinline__ tn_stream(unsigned id_, unsigned offset_, unsigned tag_, unsigned k0_, unsigned k1_)
      : id(id_), offset(offset_), tag(tag_), k0(k0_), k1(k1_), blk(0xffffffffu), w(make_uint4(0u, 0u, 0u, 0u)) {}
  __device__ __forceinline__ unsigned word(unsigned item) {         // item < 2^31: block 0xffffffff never occurs
    const unsigned b = item >> 2;
    if (b != blk) {
      w = tn_philox(b, id, offset, tag, k0, k1);
      blk = b;
    }
    return tn_lane(w, item & 3u);
  }
};

// The two unit normals of a word pair.
__device__ __forceinline__ void tn_normals(unsigned ra, unsigned rb, float& na, float& nb) {
  const float u1 = __fmul_rn((float)(2u * (ra >> 9) + 1u), TN_2M24);    // odd, below 2^24: exact, never 0
  const float a2 = __fmul_rn((float)(rb >> 8), 2.0f * TN_2M24);         // 2 u2, exact
  const float R = sqrtf(__fmul_rn(-2.0f, logf(u1)));
  na = __fmul_rn(R, cospif(a2));
  nb = __fmul_rn(R, sinpif(a2));
}

template <bool VEC>
__global__ __launch_bounds__(TN_THREADS) void taxel_noise_kernel(tn_params p) {
  unsigned k0 = p.seed_lo, k1 = p.seed_hi, off = p.offset;
  if (p.rng) {
    k0 = p.rng[0];
    k1 = p.rng[1];
    off = p.rng[2];
  }
  const long long total = p.B * p.nb;
  const long long stride = (long long)gridDim.x * TN_THREADS;
  for (long long t = (long long)blockIdx.x * TN_THREADS + threadIdx.x; t < total; t += stride) {
    const long long b = t / p.nb;
    const int j = (int)(t - b * p.nb);
    const int i0 = 4 * j;
    const int cnt = VEC ? 4 : min(4, p.CHW - i0);
    const size_t base = (size_t)b * p.CHW + i0;
    const long long id = p.ids ? p.ids[b] : p.id_base + b;
    unsigned v[4];
    if (id < 0 || id > 0x7fffffffLL) {                              // outside the contract: the sample is NaN, nothing is read
      if constexpr (VEC) {
        *reinterpret_cast<uint4*>(p.out + base) = make_uint4(TN_NAN, TN_NAN, TN_NAN, TN_NAN);
      } else {
        for (int l = 0; l < cnt; ++l) p.out[base + l] = TN_NAN;
      }
      continue;
    }
    if constexpr (VEC) {
      const uint4 q = *reinterpret_cast<const uint4*>(p.x + base);
      v[0] = q.x;
      v[1] = q.y;
      v[2] = q.z;
      v[3] = q.w;
    } else {
#pragma unroll
      for (int l = 0; l < 4; ++l) v[l] = l < cnt ? p.x[base + l] : 0u;
    }
    float n[4] = {0.f, 0.f, 0.f, 0.f};
    if (p.noise_mask) {
      const uint4 r = tn_philox((unsigned)j, (unsigned)id, off, 0u, k0, k1);
      tn_normals(r.x, r.y, n[0], n[1]);
      tn_normals(r.z, r.w, n[2], n[3]);
    }
    tn_stream gain((unsigned)id, off, 1u, k0, k1), drop((unsigned)id, off, 2u, k0, k1);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      if (l < cnt) {
        const int i = i0 + l;
        const int c = i / p.P, pix = i - c * p.P;
        const int axis = c % p.axis_cnt;
        if (p.gain_jitter != 0.f) {
          const float u = __fmul_rn((float)(gain.word((unsigned)(axis * p.P + pix)) >> 8), TN_2M24);
          const float g = fmaf(p.gain_jitter, __fsub_rn(__fmul_rn(2.0f, u), 1.0f), 1.0f);
          v[l] = __float_as_uint(__fmul_rn(g, __uint_as_float(v[l])));
        }
        if ((p.noise_mask >> axis) & 1) {
          const float val = __uint_as_float(v[l]);
          const float sa = p.sigma_add[axis];
          const float tm = __fmul_rn(p.sigma_mul[axis], val);
          const float s = sqrtf(fmaf(tm, tm, __fmul_rn(sa, sa)));
          v[l] = __float_as_uint(fmaf(s, n[l], val));
        }
        if (p.drop_thresh != 0u && (drop.word((unsigned)pix) >> 8) < p.drop_thresh) v[l] = p.drop_bits;
      }
    }
    if constexpr (VEC) {
      *reinterpret_cast<uint4*>(p.out + base) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int l = 0; l < 4; ++l)
        if (l < cnt) p.out[base + l] = v[l];
    }
  }
}

// One thread per block: the four raw words, as four dword stores (out need not be 16-byte aligned).
__global__ __launch_bounds__(TN_THREADS) void taxel_noise_bits_kernel(unsigned* out, long long B, int blocks,
                                                                      const long long* ids, long long id_base, unsigned tag,
                                                                      unsigned k0, unsigned k1, unsigned off) {
  const long long total = B * blocks;
  const long long stride = (long long)gridDim.x * TN_THREADS;
  for (long long t = (long long)blockIdx.x * TN_THREADS + threadIdx.x; t < total; t += stride) {
    const long long b = t / blocks;
    const unsigned j = (unsigned)(t - b * blocks);
    const long long id = ids ? ids[b] : id_base + b;
    uint4 r = make_uint4(TN_NAN, TN_NAN, TN_NAN, TN_NAN);
    if (id >= 0 && id <= 0x7fffffffLL) r = tn_philox(j, (unsigned)id, off, tag, k0, k1);
    unsigned* o = out + 4 * (size_t)t;
    o[0] = r.x;
    o[1] = r.y;
    o[2] = r.z;
    o[3] = r.w;
  }
}

bool tn_finite(float f) { return f - f == 0.f; }

int tn_run(const float* x, float* out, int B, int C, int H, int W, int axis_cnt, const float* sigma_add,
           const float* sigma_mul, float gain_jitter, int drop_thresh, float drop_value, const long long* ids,
           long long id_base, unsigned long long seed, unsigned offset, const unsigned* rng_dev, int max_wgs, void* stream) {
  if (!x || !out || !sigma_add || !sigma_mul) return TSR_ERR_ARG;
  if (max_wgs <= 0) return TSR_ERR_ARG;
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return TSR_ERR_ARG;
  if (axis_cnt < 1 || axis_cnt > 4 || C % axis_cnt != 0) return TSR_ERR_ARG;
  if ((long long)C * H > 0x7fffffffLL || (long long)C * H * W > 0x7fffffffLL) return TSR_ERR_ARG;
  for (int a = 0; a < axis_cnt; ++a) {
    if (!tn_finite(sigma_add[a]) || !tn_finite(sigma_mul[a]) || sigma_add[a] < 0.f || sigma_mul[a] < 0.f) return TSR_ERR_ARG;
  }
  if (!tn_finite(gain_jitter) || !tn_finite(drop_value)) return TSR_ERR_ARG;
  if (drop_thresh < 0 || drop_thresh > (1 << 24)) return TSR_ERR_ARG;
  const size_t bytes = (size_t)B * C * H * W * sizeof(float);
  const uintptr_t xa = (uintptr_t)x, oa = (uintptr_t)out;
  if (xa != oa && xa < oa + bytes && oa < xa + bytes) return TSR_ERR_ARG;       // a partial overlap
  tn_params p;
  p.x = reinterpret_cast<const unsigned*>(x);
  p.out = reinterpret_cast<unsigned*>(out);
  p.ids = ids;
  p.rng = rng_dev;
  p.id_base = id_base;
  p.B = B;
  p.P = H * W;
  p.CHW = C * H * W;
  p.nb = (int)(((long long)p.CHW + 3) / 4);
  p.axis_cnt = axis_cnt;
  p.seed_lo = (unsigned)(seed & 0xffffffffull);
  p.seed_hi = (unsigned)(seed >> 32);
  p.offset = offset;
  p.drop_thresh = (unsigned)drop_thresh;
  memcpy(&p.drop_bits, &drop_value, sizeof(float));
  p.gain_jitter = gain_jitter;
  p.noise_mask = 0;
  for (int a = 0; a < 4; ++a) {
    p.sigma_add[a] = a < axis_cnt ? sigma_add[a] : 0.f;
    p.sigma_mul[a] = a < axis_cnt ? sigma_mul[a] : 0.f;
    if (p.sigma_add[a] != 0.f || p.sigma_mul[a] != 0.f) p.noise_mask |= 1 << a;
  }
  const long long total = (long long)B * p.nb;                      // below 2^31 * 2^29
  const long long wgs = (total + TN_THREADS - 1) / TN_THREADS;
  const unsigned grid = (unsigned)(wgs > max_wgs ? max_wgs : wgs);
  const bool vec = p.P % 4 == 0 && (xa & 15) == 0 && (oa & 15) == 0;
  hipStream_t st = (hipStream_t)stream;
  if (vec) hipLaunchKernelGGL((taxel_noise_kernel<true>), dim3(grid), dim3(TN_THREADS), 0, st, p);
  else hipLaunchKernelGGL((taxel_noise_kernel<false>), dim3(grid), dim3(TN_THREADS), 0, st, p);
  return tsr_check_launch();
}

}  // namespace

extern "C" int tsr_taxel_noise_wgs(const float* x, float* out, int B, int C, int H, int W, int axis_cnt,
                                   const float* sigma_add, const float* sigma_mul, float gain_jitter, int drop_thresh,
                                   float drop_value, const long long* ids, long long id_base, unsigned long long seed,
                                   unsigned offset, int max_wgs, void* stream) {
  static_assert(TN_MAX_WGS == TSR_TAXEL_NOISE_MAX_WGS, "the default grid cap is the header's");
  return tn_run(x, out, B, C, H, W, axis_cnt, sigma_add, sigma_mul, gain_jitter, drop_thresh, drop_value, ids, id_base,
                seed, offset, nullptr, max_wgs, stream);
}

extern "C" int tsr_taxel_noise(const float* x, float* out, int B, int C, int H, int W, int axis_cnt, const float* sigma_add,
                               const float* sigma_mul, float gain_jitter, int drop_thresh, float drop_value,
                               const long long* ids, long long id_base, unsigned long long seed, unsigned offset,
                               void* stream) {
  return tn_run(x, out, B, C, H, W, axis_cnt, sigma_add, sigma_mul, gain_jitter, drop_thresh, drop_value, ids, id_base,
                seed, offset, nullptr, TN_MAX_WGS, stream);
}

extern "C" int tsr_taxel_noise_dev(const float* x, float* out, int B, int C, int H, int W, int axis_cnt,
                                   const float* sigma_add, const float* sigma_mul, float gain_jitter, int drop_thresh,
                                   float drop_value, const long long* ids, long long id_base, const unsigned* rng_dev,
                                   void* stream) {
  if (!rng_dev) return TSR_ERR_ARG;
  return tn_run(x, out, B, C, H, W, axis_cnt, sigma_add, sigma_mul, gain_jitter, drop_thresh, drop_value, ids, id_base,
                0ull, 0u, rng_dev, TN_MAX_WGS, stream);
}

extern "C" int tsr_taxel_noise_bits(unsigned* out, int B, int blocks, const long long* ids, long long id_base, int tag,
                                    unsigned long long seed, unsigned offset, void* stream) {
  if (!out || B <= 0 || blocks <= 0 || tag < 0) return TSR_ERR_ARG;
  const long long total = (long long)B * blocks;
  const long long wgs = (total + TN_THREADS - 1) / TN_THREADS;
  const unsigned grid = (unsigned)(wgs > TN_MAX_WGS ? TN_MAX_WGS : wgs);
  hipLaunchKernelGGL(taxel_noise_bits_kernel, dim3(grid), dim3(TN_THREADS), 0, (hipStream_t)stream, out, (long long)B, blocks,
                     ids, id_base, (unsigned)tag, (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), offset);
  return tsr_check_launch();
}
