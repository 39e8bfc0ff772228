// Host-side layer shared by the convolution launchers: the prototypes of every internal (non-extern "C") function that
// crosses translation units, the one argument check + ConvArgs fill of the conv entry points, the one (cout, ks) launch
// ladder and the grid of the weight-pack kernels.  Host only: nothing here is __global__ or __device__.  The defining
// files include it too, so a prototype that drifts from its definition is a compile error.
#pragma once
#include "tsr_common.h"
#include "conv_args.h"
#include <type_traits>

// ---- conv_mfma_k32.hip (fp16x3 3x3 / 5x5, 16x16x32 MFMA) -------------------------------------------------------------
int tsr_conv_k32(const ConvArgs& a, int cout, int ks, bool ext, hipStream_t st);
int tsr_conv_k32_fuse1x1(const ConvArgs& a, int ks, hipStream_t st);
int tsr_conv_k32_images(int cout);              // images per workgroup of the plain / training launches
// ---- conv_mfma_split16.hip -------------------------------------------------------------------------------------------
int tsr_conv_f16s_images(int cout, int ks);     // images per workgroup of the fp16x3 kernel that runs (cout, ks)
int tsr_conv2d_ex_bf16s(const ConvArgs& a, int cout, int ks, int nsplit, hipStream_t st);      // tsr_conv2d_ex, nsplit != 0
// ---- conv_b16k.hip / conv1x1_b16k.hip (bf16 storage, LDS-DMA) --------------------------------------------------------
int tsr_conv_b16k_ex(const ConvArgs& a, int cout, int ks, bool pair, hipStream_t st);          // nsplit = -3 / -4
int tsr_conv_b16k_images();                     // images per workgroup of every conv_b16k launch
int tsr_dgrad1x1_b16k(const ConvArgs& a, hipStream_t st);
int tsr_fwd1x1_b16k(const ConvArgs& a, int cout, hipStream_t st);
int tsr_dgrad1x1_b16k_grid(int B, int H, int W);
// ---- wgrad_b16k.hip --------------------------------------------------------------------------------------------------
bool tsr_wgrad_b16k_ok(int cout, int cin, int ks, int H, int W, int a_ctot, int dz_ctot);
int tsr_wgrad_b16k_1x1_wgs(int cout, int cin);
int tsr_wgrad_b16k(const void* a, int a_ctot, int a_coff, int cin, const float* a_scale, const float* a_shift, const void* dz,
                   int dz_ctot, int dz_coff, int cout, int ks, float* slab, float* bias_slab, int nsplit, int B, int H, int W,
                   hipStream_t st);

// The argument check every conv entry point shares, and the common part of its ConvArgs: required pointers, B / H / W > 0,
// cin > 0, every channel count and offset a multiple of 16, no negative offset, the in / out / res slices inside their
// buffers (`out_ch` = the width of `out` and `res`; `res` is checked only when given).  Zero-initialises `a`, so the
// extension fields an entry point does not set mean "inference behaviour".  TSR_ERR_ARG = refused, `a` untouched.
static inline int conv_fill(ConvArgs& a, const void* in, int in_ctot, int in_coff, int cin, const void* w_packed,
                            const float* scale, const float* shift, const void* res, int res_ctot, int res_coff, void* out,
                            int out_ctot, int out_coff, int out_ch, int relu, int B, int H, int W) {
  if (!in || !w_packed || !out || B <= 0 || H <= 0 || W <= 0) return TSR_ERR_ARG;
  if ((cin & 15) || (in_ctot & 15) || (in_coff & 15) || (out_ctot & 15) || (out_coff & 15) || cin <= 0 ||
      in_coff < 0 || out_coff < 0 || in_coff + cin > in_ctot || out_coff + out_ch > out_ctot)
    return TSR_ERR_ARG;
  if (res && ((res_ctot & 15) || (res_coff & 15) || res_coff < 0 || res_coff + out_ch > res_ctot)) return TSR_ERR_ARG;
  a = ConvArgs{};
  a.in = (const float*)in; a.in_ctot = in_ctot; a.in_coff = in_coff; a.cin = cin;
  a.wp = (const float*)w_packed; a.scale = scale; a.shift = shift;
  a.res = (const float*)res; a.res_ctot = res_ctot; a.res_coff = res_coff;
  a.out = (float*)out; a.out_ctot = out_ctot; a.out_coff = out_coff; a.relu = relu;
  a.B = B; a.H = H; a.W = W;
  a.tiles_x = (W + 7) / 8; a.tiles_y = (H + 7) / 8;
  return TSR_OK;
}

// The fp16x3 launches' own rule (conv_mfma_split16.hip, conv_mfma_k32.hip): the input's amax slot and a positive weight
// scale (a NaN is refused)
static inline bool f16s_scales_ok(const float* in_amax, float w_inv_scale) { return in_amax && w_inv_scale > 0.f; }

// The one (cout, ks) ladder: f(integral_constant<COUT>, integral_constant<KS>) for cout in {64, 128}, ks in {1, 3, 5},
// TSR_ERR_ARG for every other pair.  A family without a ks = 1 kernel guards its call with `if constexpr`.  FIRST = the
// width whose forms are instantiated first: it decides nothing but the order of a file's kernels in its code object
// (conv_b16k.hip has always listed its 128-channel forms first and passes 128 to keep its code object as it is).
template <int V> using tsr_ic = std::integral_constant<int, V>;
template <int FIRST = 64, class F> static inline int for_cout_ks(int cout, int ks, F&& f) {
  constexpr int SECOND = 192 - FIRST;
  static_assert(FIRST == 64 || FIRST == 128, "the conv kernels have 64 or 128 output channels");
  if (cout == FIRST) {
    if (ks == 1) return f(tsr_ic<FIRST>{}, tsr_ic<1>{});
    if (ks == 3) return f(tsr_ic<FIRST>{}, tsr_ic<3>{});
    if (ks == 5) return f(tsr_ic<FIRST>{}, tsr_ic<5>{});
  } else if (cout == SECOND) {
    if (ks == 1) return f(tsr_ic<SECOND>{}, tsr_ic<1>{});
    if (ks == 3) return f(tsr_ic<SECOND>{}, tsr_ic<3>{});
    if (ks == 5) return f(tsr_ic<SECOND>{}, tsr_ic<5>{});
  }
  return TSR_ERR_ARG;
}

// Shapes the weight packs of the 64 / 128-channel conv kernels take: the forward conv, and the dgrad conv that produces
// the gradient of input channels [ci0, ci0 + nprime) of a conv with OIHW weight [cout][cin][ks][ks].
static inline bool pack_shape_ok(int cout, int cin, int ks) {
  return cin > 0 && !(cin & 15) && (cout == 64 || cout == 128) && (ks == 1 || ks == 3 || ks == 5);
}
static inline bool pack_dgrad_shape_ok(int cout, int cin, int ks, int ci0, int nprime) {
  return !(cout & 15) && (nprime == 64 || nprime == 128) && ci0 >= 0 && ci0 + nprime <= cin && (ks == 1 || ks == 3 || ks == 5);
}
// grid of a grid-stride pack kernel: one 256-thread workgroup per 256 elements, 4096 workgroups at most
static inline dim3 pack_grid(size_t total) {
  const int grid = (int)((total + 255) / 256);
  return dim3(grid > 4096 ? 4096 : grid);
}
