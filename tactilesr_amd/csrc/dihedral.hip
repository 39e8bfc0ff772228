// Rot90 / flip augmentation on the device: gather sample idx[b] and write it already transformed by one of the eight
// dihedral ops (tsr_gather_dihedral, include/tactilesr_hip.h).
//
//   out[b] = (accumulate ? out[b] : 0) + scale * D_{op[b]}( src[ idx ? idx[b] : b ] )        b < B
//
// With op = k + 4 f (f: mirror along W first, then k counter-clockwise quarter turns as np.rot90) the element (i, j) of
// an output plane comes from the source element
//   (r, c) = (a(u), b(v)),  (u, v) = k odd ? (j, i) : (i, j),  a(u) = [op & 2] ? H-1-u : u,  b(v) = [popcount(op) odd] ? W-1-v : v
// so even k only reverses rows and / or columns and odd k is a transpose with the same two reversals.
//
// Three kernels, each a walk over work items that puts everything scaling with B into grid x:
//   * planes of at most 64 elements (the 4x4 taxels): one thread per output element, direct reads;
//   * planes whose H rows of W + 1 dwords fit 62 KiB of LDS (up to 125 x 125: every shape of the project): one workgroup
//     of 256 per plane of one sample, the op uniform per workgroup.  Even k: one pass over the output plane in memory
//     order, each item read from its mirrored row / column position (reversed in registers when columns flip); no LDS.
//     Odd k: the source plane is read in ITS memory order into LDS (row pitch W + 1), then the output plane is written in
//     memory order from LDS columns.  Both global passes are linear over whole planes, so every cache line is read and
//     written whole and by one workgroup -- tiles of a 100-wide plane cut each 400-byte row into pieces that start and
//     end inside cache lines, and hand the pieces of one line to different workgroups.
//     A thread issues five loads (half of its share of a 100x100 plane) before its first store.  LDS: a float4 item is
//     four dword accesses, lanes 4 dwords (or 4 pitches) apart: 8 banks per half-wave, a 4-way conflict, ~2.5 k LDS cycles
//     per 100x100 plane against ~9 k cycles of HBM time per plane and CU.
//   * larger planes: a workgroup of 256 takes one 64 x 64 tile of one plane of one sample; the op is uniform per tile.
//     A thread moves four float4 (rows a, a+16, a+32, a+48 of the tile; all four loads are issued before the first store:
//     with one load per thread the launch is bound by the bytes in flight, not by HBM).  Even k: rows stay rows, the
//     four floats are reversed in registers when columns flip; no LDS.  Odd k: the source tile is read along ITS rows
//     into LDS (row pitch 65 dwords), then read back transposed, so the global writes run along rows too.  With the
//     pitch = 1 mod 32 the 32 lanes of a half-wave that read a column with float4 granularity (16 column groups x 2 rows)
//     fall on 16 banks, two lanes each: a 2-way conflict on 16 KiB of LDS traffic per tile, far below the HBM time.
//   * the tile kernel moves float4 where src, out are 16-byte aligned and W % 4 == 0 (then every plane and row is), and
//     one float per lane, 64 consecutive lanes on a row (conflict-free in LDS), otherwise.
// No atomics; an output element is written by one thread: two launches give the same bits.  Data move as 32-bit patterns:
// with scale == 1 and no accumulation nothing is computed and NaN payloads survive; a negative csign flips the sign bit.
#include "tsr_common.h"
#include "tactilesr_hip.h"

namespace {

constexpr int DH_THREADS = 256;
constexpr int DH_TILE = 64;
constexpr int DH_PITCH = DH_TILE + 1;               // dwords; 65 = 1 mod 32
constexpr int DH_VROWS = DH_THREADS / (DH_TILE / 4);  // rows one pass of float4 covers: 16
constexpr int DH_VPASS = DH_TILE / DH_VROWS;          // 4
constexpr int DH_SROWS = DH_THREADS / DH_TILE;        // rows one pass of single floats covers: 4
constexpr int DH_SPASS = DH_TILE / DH_SROWS;          // 16
constexpr int DH_SMALL = 64;                        // planes up to this many elements go one thread per element
constexpr int DH_PLANE_LDS = 15872;                 // dwords (62 KiB): planes with H * (W + 1) up to this go one workgroup a plane
constexpr int DH_UNROLL = 5;                        // items a thread of the plane kernel loads before its first store
constexpr int DH_MAX_WGS = 1 << 20;                 // tsr_gather_dihedral's grid cap (TSR_DIHEDRAL_MAX_WGS): a workgroup walks further items
constexpr unsigned DH_NAN = 0x7fc00000u;

struct dh_params {
  const unsigned* src;
  unsigned* out;
  const long long* idx;
  const int* op;
  const int* cmap;
  const float* csign;
  long long n_src;
  int B, C, H, W;
  int op_all, op_mask;
  float scale;
};

// The op and source sample of output sample b; false when a device value is outside the contract (the sample is NaN).
__device__ __forceinline__ bool dh_sample(const dh_params& p, long long b, int& op, long long& s) {
  op = p.op ? p.op[b] : p.op_all;
  s = p.idx ? p.idx[b] : b;
  return (unsigned)op < 8u && ((p.op_mask >> op) & 1) && s >= 0 && s < p.n_src;
}

// The source channel and sign-bit flip of output channel c under a valid op.
__device__ __forceinline__ bool dh_channel(const dh_params& p, int op, int c, int& sc, unsigned& flip) {
  sc = c;
  flip = 0u;
  if (p.cmap) {
    sc = p.cmap[op * p.C + c];
    flip = __float_as_uint(p.csign[op * p.C + c]) & 0x80000000u;
  }
  return (unsigned)sc < (unsigned)p.C;
}

// MODE 0: the bits; 1: one rounding of scale * x; 2: one fma onto the prior.
template <int MODE>
__device__ __forceinline__ unsigned dh_value(unsigned x, unsigned flip, float scale, unsigned prior) {
  x ^= flip;
  if constexpr (MODE == 0) return x;
  else if constexpr (MODE == 1) return __float_as_uint(scale * __uint_as_float(x));
  else return __float_as_uint(fmaf(scale, __uint_as_float(x), __uint_as_float(prior)));
}

template <int MODE>
__global__ __launch_bounds__(DH_THREADS) void dihedral_small_kernel(dh_params p, size_t total) {
  const int HW = p.H * p.W;
  const size_t CHW = (size_t)p.C * HW;
  const size_t stride = (size_t)gridDim.x * DH_THREADS;
  for (size_t e = (size_t)blockIdx.x * DH_THREADS + threadIdx.x; e < total; e += stride) {
    const size_t plane = e / HW;
    const int pix = (int)(e - plane * HW);
    const int c = (int)(plane % p.C);
    const long long b = (long long)(plane / p.C);
    const int i = pix / p.W, j = pix - i * p.W;
    int op, sc = 0;
    long long s;
    unsigned flip = 0u;
    bool ok = dh_sample(p, b, op, s);
    if (ok) ok = dh_channel(p, op, c, sc, flip);
    if (!ok) {
      p.out[e] = DH_NAN;
      continue;
    }
    const bool tr = op & 1, fr = (op >> 1) & 1, fc = __popc(op) & 1;
    const int u = tr ? j : i, v = tr ? i : j;                  // odd k only with H == W
    const int r = fr ? p.H - 1 - u : u, cc = fc ? p.W - 1 - v : v;
    const unsigned x = p.src[(size_t)s * CHW + (size_t)sc * HW + r * p.W + cc];
    p.out[e] = dh_value<MODE>(x, flip, p.scale, MODE == 2 ? p.out[e] : 0u);
  }
}

__device__ __forceinline__ uint4 dh_rev(const uint4& v) { return make_uint4(v.w, v.z, v.y, v.x); }

template <int MODE>
__device__ __forceinline__ void dh_store4(unsigned* o, uint4 v, unsigned flip, float scale) {
  uint4 prior = make_uint4(0u, 0u, 0u, 0u);
  if constexpr (MODE == 2) prior = *reinterpret_cast<const uint4*>(o);
  *reinterpret_cast<uint4*>(o) = make_uint4(dh_value<MODE>(v.x, flip, scale, prior.x), dh_value<MODE>(v.y, flip, scale, prior.y),
                                            dh_value<MODE>(v.z, flip, scale, prior.z), dh_value<MODE>(v.w, flip, scale, prior.w));
}

template <int MODE, bool VEC>
__global__ __launch_bounds__(DH_THREADS) void dihedral_tile_kernel(dh_params p, long long ntiles, int TH, int TW) {
  __shared__ unsigned lds[DH_TILE * DH_PITCH];
  const int H = p.H, W = p.W, HW = H * W;
  const size_t CHW = (size_t)p.C * HW;
  const int tid = threadIdx.x;
  // VEC: thread = (rows a + 16 m, 4 columns from q); scalar: thread = (rows g + 4 m, column lane)
  const int a = tid / (DH_TILE / 4), q = (tid % (DH_TILE / 4)) * 4;
  const int g = tid / DH_TILE, lane = tid % DH_TILE;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int tj = (int)(t % TW);
    long long rest = t / TW;
    const int ti = (int)(rest % TH);
    rest /= TH;
    const int c = (int)(rest % p.C);
    const long long b = rest / p.C;
    const int i0 = ti * DH_TILE, j0 = tj * DH_TILE;
    unsigned* o = p.out + (size_t)b * CHW + (size_t)c * HW;
    int op, sc = 0;
    long long s;
    unsigned flip = 0u;
    bool ok = dh_sample(p, b, op, s);                            // uniform over the workgroup
    if (ok) ok = dh_channel(p, op, c, sc, flip);
    if (!ok) {
      if constexpr (VEC) {
#pragma unroll
        for (int m = 0; m < DH_VPASS; ++m) {
          const int i = i0 + a + DH_VROWS * m, j = j0 + q;
          if (i < H && j < W) *reinterpret_cast<uint4*>(o + i * W + j) = make_uint4(DH_NAN, DH_NAN, DH_NAN, DH_NAN);
        }
      } else {
#pragma unroll
        for (int m = 0; m < DH_SPASS; ++m) {
          const int i = i0 + g + DH_SROWS * m, j = j0 + lane;
          if (i < H && j < W) o[i * W + j] = DH_NAN;
        }
      }
      continue;
    }
    const unsigned* x = p.src + (size_t)s * CHW + (size_t)sc * HW;
    const bool tr = op & 1, fr = (op >> 1) & 1, fc = __popc(op) & 1;
    if (!tr) {
      if constexpr (VEC) {
        uint4 v[DH_VPASS];
        const int j = j0 + q;                                    // W % 4 == 0: the four columns are inside together
#pragma unroll
        for (int m = 0; m < DH_VPASS; ++m) {
          const int i = i0 + a + DH_VROWS * m;
          if (i < H && j < W) v[m] = *reinterpret_cast<const uint4*>(x + (fr ? H - 1 - i : i) * W + (fc ? W - 4 - j : j));
        }
#pragma unroll
        for (int m = 0; m < DH_VPASS; ++m) {
          const int i = i0 + a + DH_VROWS * m;
          if (i < H && j < W) dh_store4<MODE>(o + i * W + j, fc ? dh_rev(v[m]) : v[m], flip, p.scale);
        }
      } else {
        unsigned v[DH_SPASS];
        const int j = j0 + lane, cc = fc ? W - 1 - j : j;
#pragma unroll
        for (int m = 0; m < DH_SPASS; ++m) {
          const int i = i0 + g + DH_SROWS * m;
          if (i < H && j < W) v[m] = x[(fr ? H - 1 - i : i) * W + cc];
        }
#pragma unroll
        for (int m = 0; m < DH_SPASS; ++m) {
          const int i = i0 + g + DH_SROWS * m;
          if (i < H && j < W) {
            unsigned* d = o + i * W + j;
            *d = dh_value<MODE>(v[m], flip, p.scale, MODE == 2 ? *d : 0u);
          }
        }
      }
    } else {                                                     // H == W: out (i, j) <- src (a(j), b(i))
      if constexpr (VEC) {
        uint4 v[DH_VPASS];
        const int ii = i0 + q;                                   // source columns from ii .. ii + 3, source rows from jj
#pragma unroll
        for (int m = 0; m < DH_VPASS; ++m) {
          const int jj = j0 + a + DH_VROWS * m;
          if (jj < W && ii < H) v[m] = *reinterpret_cast<const uint4*>(x + (fr ? H - 1 - jj : jj) * W + (fc ? W - 4 - ii : ii));
        }
#pragma unroll
        for (int m = 0; m < DH_VPASS; ++m) {
          const int jl = a + DH_VROWS * m;
          if (j0 + jl < W && ii < H) {
            const uint4 w = fc ? dh_rev(v[m]) : v[m];
            unsigned* l = lds + jl * DH_PITCH + q;               // lds[j - j0][i - i0]
            l[0] = w.x;
            l[1] = w.y;
            l[2] = w.z;
            l[3] = w.w;
          }
        }
        __syncthreads();
        const int j = j0 + q;
#pragma unroll
        for (int m = 0; m < DH_VPASS; ++m) {
          const int il = a + DH_VROWS * m, i = i0 + il;
          if (i < H && j < W) {
            const unsigned* l = lds + q * DH_PITCH + il;
            dh_store4<MODE>(o + i * W + j, make_uint4(l[0], l[DH_PITCH], l[2 * DH_PITCH], l[3 * DH_PITCH]), flip, p.scale);
          }
        }
      } else {
        const int ii = i0 + lane, cc = fc ? W - 1 - ii : ii;
#pragma unroll
        for (int m = 0; m < DH_SPASS; ++m) {
          const int jl = g + DH_SROWS * m, jj = j0 + jl;
          if (jj < W && ii < H) lds[jl * DH_PITCH + lane] = x[(fr ? H - 1 - jj : jj) * W + cc];
        }
        __syncthreads();
        const int j = j0 + lane;
#pragma unroll
        for (int m = 0; m < DH_SPASS; ++m) {
          const int il = g + DH_SROWS * m, i = i0 + il;
          if (i < H && j < W) {
            unsigned* d = o + i * W + j;
            *d = dh_value<MODE>(lds[lane * DH_PITCH + il], flip, p.scale, MODE == 2 ? *d : 0u);
          }
        }
      }
      __syncthreads();                                           // the next tile of the walk rewrites lds
    }
  }
}

// What a thread of the plane kernel moves at a time: four consecutive floats of a row, or one.
template <bool VEC>
struct dh_item;
template <>
struct dh_item<true> {
  uint4 v;
  __device__ __forceinline__ void load(const unsigned* g) { v = *reinterpret_cast<const uint4*>(g); }
  __device__ __forceinline__ void reverse() { v = dh_rev(v); }
  template <int MODE>
  __device__ __forceinline__ void store(unsigned* o, unsigned flip, float scale) const {
    dh_store4<MODE>(o, v, flip, scale);
  }
  __device__ __forceinline__ void to_lds(unsigned* l) const {
    l[0] = v.x;
    l[1] = v.y;
    l[2] = v.z;
    l[3] = v.w;
  }
  __device__ __forceinline__ void from_lds_column(const unsigned* l, int step) {
    v = make_uint4(l[0], l[step], l[2 * step], l[3 * step]);
  }
};
template <>
struct dh_item<false> {
  unsigned v;
  __device__ __forceinline__ void load(const unsigned* g) { v = *g; }
  __device__ __forceinline__ void reverse() {}
  template <int MODE>
  __device__ __forceinline__ void store(unsigned* o, unsigned flip, float scale) const {
    *o = dh_value<MODE>(v, flip, scale, MODE == 2 ? *o : 0u);
  }
  __device__ __forceinline__ void to_lds(unsigned* l) const { *l = v; }
  __device__ __forceinline__ void from_lds_column(const unsigned* l, int) { v = *l; }
};

// One workgroup per plane: every global read and write is one linear pass over the plane.
template <int MODE, bool VEC>
__global__ __launch_bounds__(DH_THREADS) void dihedral_plane_kernel(dh_params p, long long nplanes) {
  extern __shared__ unsigned lds[];                              // H * (W + 1) dwords: the launch sizes it to the plane
  const int H = p.H, W = p.W, HW = H * W, P = W + 1;
  constexpr int K = VEC ? 4 : 1;                                 // floats per item
  const int WK = W / K, n = HW / K;                              // items per row, per plane
  const int tid = threadIdx.x;
  for (long long pl = blockIdx.x; pl < nplanes; pl += gridDim.x) {
    const int c = (int)(pl % p.C);
    const long long b = pl / p.C;
    unsigned* o = p.out + (size_t)pl * HW;                       // planes of out follow each other
    int op, sc = 0;
    long long s;
    unsigned flip = 0u;
    bool ok = dh_sample(p, b, op, s);                            // uniform over the workgroup
    if (ok) ok = dh_channel(p, op, c, sc, flip);
    if (!ok) {
      for (int v = tid; v < n; v += DH_THREADS) {
        if constexpr (VEC) *reinterpret_cast<uint4*>(o + 4 * v) = make_uint4(DH_NAN, DH_NAN, DH_NAN, DH_NAN);
        else o[v] = DH_NAN;
      }
      continue;
    }
    const unsigned* x = p.src + ((size_t)s * p.C + sc) * HW;
    const bool tr = op & 1, fr = (op >> 1) & 1, fc = __popc(op) & 1;
    if (!tr) {
      for (int v0 = tid; v0 < n; v0 += DH_UNROLL * DH_THREADS) {
        dh_item<VEC> val[DH_UNROLL];
#pragma unroll
        for (int u = 0; u < DH_UNROLL; ++u) {
          const int v = v0 + u * DH_THREADS;
          if (v < n) {
            const int i = v / WK, jk = v - i * WK;
            val[u].load(x + (fr ? H - 1 - i : i) * W + K * (fc ? WK - 1 - jk : jk));
          }
        }
#pragma unroll
        for (int u = 0; u < DH_UNROLL; ++u) {
          const int v = v0 + u * DH_THREADS;
          if (v < n) {
            if (fc) val[u].reverse();
            val[u].template store<MODE>(o + K * v, flip, p.scale);
          }
        }
      }
    } else {                                                     // H == W: out (i, j) <- src (a(j), b(i)), through lds[r][c]
      for (int v0 = tid; v0 < n; v0 += DH_UNROLL * DH_THREADS) {
        dh_item<VEC> val[DH_UNROLL];
#pragma unroll
        for (int u = 0; u < DH_UNROLL; ++u) {
          const int v = v0 + u * DH_THREADS;
          if (v < n) val[u].load(x + K * v);
        }
#pragma unroll
        for (int u = 0; u < DH_UNROLL; ++u) {
          const int v = v0 + u * DH_THREADS;
          if (v < n) {
            const int r = v / WK, ck = v - r * WK;
            val[u].to_lds(lds + r * P + K * ck);
          }
        }
      }
      __syncthreads();
      for (int v = tid; v < n; v += DH_THREADS) {
        const int i = v / WK, j = K * (v - i * WK);
        const unsigned* l = lds + (fc ? W - 1 - i : i);           // column b(i); rows a(j), a(j + 1), ..
        dh_item<VEC> val;
        val.from_lds_column(l + (fr ? H - 1 - j : j) * P, fr ? -P : P);
        val.template store<MODE>(o + K * v, flip, p.scale);
      }
      __syncthreads();                                           // the next plane of the walk rewrites lds
    }
  }
}

template <int MODE>
void dh_launch(const dh_params& p, long long max_wgs, hipStream_t st) {
  const long long HW = (long long)p.H * p.W;
  if (HW <= DH_SMALL) {
    const size_t total = (size_t)p.B * p.C * HW;
    const long long wgs = (long long)((total + DH_THREADS - 1) / DH_THREADS);
    const unsigned grid = (unsigned)(wgs > max_wgs ? max_wgs : wgs);
    hipLaunchKernelGGL((dihedral_small_kernel<MODE>), dim3(grid), dim3(DH_THREADS), 0, st, p, total);
    return;
  }
  if (HW + p.H <= DH_PLANE_LDS) {                                // H rows of W + 1 dwords fit the LDS array
    const long long nplanes = (long long)p.B * p.C;
    const unsigned grid = (unsigned)(nplanes > max_wgs ? max_wgs : nplanes);
    const bool vec = p.W % 4 == 0 && ((uintptr_t)p.src & 15) == 0 && ((uintptr_t)p.out & 15) == 0;
    const size_t lds = (size_t)(HW + p.H) * sizeof(unsigned);   // 40.4 KB for 100x100: three workgroups a CU
    if (vec) hipLaunchKernelGGL((dihedral_plane_kernel<MODE, true>), dim3(grid), dim3(DH_THREADS), lds, st, p, nplanes);
    else hipLaunchKernelGGL((dihedral_plane_kernel<MODE, false>), dim3(grid), dim3(DH_THREADS), lds, st, p, nplanes);
    return;
  }
  const int TH = (p.H + DH_TILE - 1) / DH_TILE, TW = (p.W + DH_TILE - 1) / DH_TILE;
  const long long ntiles = (long long)p.B * p.C * TH * TW;      // B < 2^31 and C * TH * TW <= C*H*W < 2^31: below 2^62
  const unsigned grid = (unsigned)(ntiles > max_wgs ? max_wgs : ntiles);
  const bool vec = p.W % 4 == 0 && ((uintptr_t)p.src & 15) == 0 && ((uintptr_t)p.out & 15) == 0;
  if (vec)
    hipLaunchKernelGGL((dihedral_tile_kernel<MODE, true>), dim3(grid), dim3(DH_THREADS), 0, st, p, ntiles, TH, TW);
  else
    hipLaunchKernelGGL((dihedral_tile_kernel<MODE, false>), dim3(grid), dim3(DH_THREADS), 0, st, p, ntiles, TH, TW);
}

}  // namespace

extern "C" int tsr_gather_dihedral_wgs(const float* src, int n_src, const long long* idx, const int* op, int op_all,
                                       int op_mask, const int* cmap, const float* csign, float* out, int B, int C, int H,
                                       int W, float scale, int accumulate, int max_wgs, void* stream) {
  static_assert(DH_MAX_WGS == TSR_DIHEDRAL_MAX_WGS, "the default grid cap is the header's");
  if (!src || !out) return TSR_ERR_ARG;
  if (max_wgs <= 0) return TSR_ERR_ARG;
  if (B <= 0 || n_src <= 0 || C <= 0 || H <= 0 || W <= 0) return TSR_ERR_ARG;
  if (op_mask <= 0 || op_mask > 0xff) return TSR_ERR_ARG;
  if ((op_mask & 0xaa) && H != W) return TSR_ERR_ARG;                    // an odd k turns H x W into W x H
  if (!op && (op_all < 0 || op_all > 7 || !((op_mask >> op_all) & 1))) return TSR_ERR_ARG;
  if ((cmap == nullptr) != (csign == nullptr)) return TSR_ERR_ARG;
  if (accumulate != 0 && accumulate != 1) return TSR_ERR_ARG;
  if (scale != scale) return TSR_ERR_ARG;
  if ((long long)C * H > 0x7fffffffLL || (long long)C * H * W > 0x7fffffffLL) return TSR_ERR_ARG;
  dh_params p;
  p.src = reinterpret_cast<const unsigned*>(src);
  p.out = reinterpret_cast<unsigned*>(out);
  p.idx = idx;
  p.op = op;
  p.cmap = cmap;
  p.csign = csign;
  p.n_src = n_src;
  p.B = B;
  p.C = C;
  p.H = H;
  p.W = W;
  p.op_all = op_all;
  p.op_mask = op_mask;
  p.scale = scale;
  hipStream_t st = (hipStream_t)stream;
  if (accumulate) dh_launch<2>(p, max_wgs, st);
  else if (scale == 1.0f) dh_launch<0>(p, max_wgs, st);
  else dh_launch<1>(p, max_wgs, st);
  return tsr_check_launch();
}

extern "C" int tsr_gather_dihedral(const float* src, int n_src, const long long* idx, const int* op, int op_all,
                                   int op_mask, const int* cmap, const float* csign, float* out, int B, int C, int H,
                                   int W, float scale, int accumulate, void* stream) {
  return tsr_gather_dihedral_wgs(src, n_src, idx, op, op_all, op_mask, cmap, csign, out, B, C, H, W, scale, accumulate,
                                 DH_MAX_WGS, stream);
}
