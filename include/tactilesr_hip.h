/* tactilesr_hip.h -- C ABI of libtactilesr_hip.so (MI355X / gfx950 only).
 *
 * The reference (wmtlab/tactileSR) has no FFI of its own: its hot path is the set of
 * torch.nn / torch.nn.functional calls issued by model/tactileSR_model.py and
 * model/tPSFNet.py.  Each entry point below replaces one group of those calls; the
 * reference line(s) it stands in for are cited per function.  INTEGRATION.md shows the
 * ctypes binding a maintainer adds on the reference side.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (PyTorch): the library never
 *    allocates, frees or retains memory; `stream` is a hipStream_t (0 = null stream);
 *    all work is enqueued asynchronously on it;
 *  - return value: 0 = TSR_OK, 1 = bad argument, 2 = launch failure; no exceptions;
 *  - "CB16" = the internal channel-blocked activation layout float[B][C/16][H*W][16];
 *    `ctot` is the channel count of the whole buffer, `coff` the first channel touched
 *    (both multiples of 16) -- producers write straight into channel slices of the
 *    consumer's buffer, which is how every torch.cat of the reference is elided
 *    (model/tactileSR_model.py:74,81,200,203);
 *  - boundary tensors are NCHW fp32 contiguous, as the reference's callers pass them
 *    (train/tactileSR_train.py:43-47).
 */
#ifndef TACTILESR_HIP_H
#define TACTILESR_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

#define TSR_OK 0
#define TSR_ERR_ARG 1
#define TSR_ERR_LAUNCH 2

/* Library / ABI version (bumped on any signature change). */
int tsr_abi_version(void);

/* 0 for the shipped library; non-zero for an experimental variant built by tools/build_variant.py (extra -D flags).  The
 * Python binding refuses a non-zero library unless TSR_ALLOW_VARIANT=1 is set, and bench.py reports the value. */
int tsr_build_flags(void);

/* Re-order an nn.Conv2d weight (OIHW fp32; Cout in {64,128}, Cin % 16 == 0, k in {1,3,5})
 * into the [Cin/16][k*k][4][Cout][4] stream order tsr_conv2d_fwd consumes.
 * w_packed holds Cout*Cin*k*k floats.  Status 1 and no launch for a NULL pointer, cin <= 0 or a shape outside the above
 * (tsr_pack_conv_weight_bf16s alike); the full list of refusals is in the "Refusals" paragraph at tsr_conv2d_fwd_bf16s below. */
int tsr_pack_conv_weight(const float* w_oihw, float* w_packed, int cout, int cin, int ks, void* stream);

/* out[:, coff:coff+cout] = act( conv2d(in[:, in_coff:in_coff+cin], W, stride 1, pad k/2) * scale + shift
 *                               (+ res[:, res_coff:res_coff+cout]) ),  act = ReLU if relu else identity.
 * Replaces nn.Conv2d (+bias) + nn.BatchNorm2d(eval) + nn.ReLU / residual add of
 *   MSRB   model/tactileSR_model.py:167-191,196-206   (conv_3_1, conv_5_1, conv_3_2, conv_5_2, confusion,
 *                                                      `output += x`, relu)
 *   ResBlock                     :219-225
 *   stem conv2 / inputContact_layer / output_layer[0]  :41-43,47-49,53-54
 * scale/shift are per-output-channel (NULL = 1 / 0): eval-mode BN folds to
 *   scale = gamma/sqrt(running_var+eps), shift = (bias-running_mean)*scale+beta.
 * in/out/res are CB16; fp32 MFMA (exact fp32 fma chain).
 * tsr_conv2d_fwd, tsr_conv2d_fwd_bf16s and tsr_conv2d_ex refuse (status 1, nothing launched) a NEGATIVE channel offset like
 * any other slice that leaves its buffer: in_coff, out_coff and -- when the tensor is given -- res_coff (tsr_conv2d_ex: and
 * mask_coff).  Every refusal of tsr_conv2d_fwd is listed in the "Refusals" paragraph at tsr_conv2d_fwd_bf16s below. */
int tsr_conv2d_fwd(const float* in, int in_ctot, int in_coff, int cin,
                   const float* w_packed, int cout, int ks,
                   const float* scale, const float* shift,
                   const float* res, int res_ctot, int res_coff,
                   float* out, int out_ctot, int out_coff, int relu,
                   int B, int H, int W, void* stream);

/* Split-bf16 variant of tsr_conv2d_fwd on the bf16 matrix cores (16x the fp32-MFMA rate on gfx950):
 * fp32 operands are split into nsplit bf16 planes and the significant cross products are accumulated in
 * fp32.  nsplit = 3 ("bf16x6": 6 products, 24 significand bits -> fp32-equivalent results, error <= the fp32
 * MFMA path's); nsplit = 2 ("bf16x3": 3 products, ~4e-6 per layer); nsplit = 1 (plain bf16 operands).
 * Same arguments and semantics as tsr_conv2d_fwd; weights come from tsr_pack_conv_weight_bf16s
 * (tsr_conv_weight_bf16s_elems() bf16 values: taps padded to the kernel's step size).
 * Refusals (status 1, nothing is launched, `out` is untouched) of tsr_conv2d_fwd and tsr_conv2d_fwd_bf16s (checked launch by
 * launch in tests/test_gpu_infer_f32s.py, without a device in tests/test_infer_f32s_cpu.py): a NULL in, w_packed or out; B, H
 * or W <= 0; cin <= 0; cin, any ctot or any coff not a multiple of 16; a negative coff or a slice that leaves its buffer
 * (coff + channels > ctot) for in, out and -- when res is given -- res; cout not in {64, 128}; ks not in {1, 3, 5};
 * tsr_conv2d_fwd_bf16s: nsplit not in {1, 2, 3}.  scale, shift and res may each be NULL on their own (1 / 0 / no residual;
 * res_ctot and res_coff are then ignored).  tsr_pack_conv_weight and tsr_pack_conv_weight_bf16s refuse a NULL pointer, cin <= 0
 * or not a multiple of 16, cout not in {64, 128}, ks not in {1, 3, 5} and (_bf16s) nsplit not in {1, 2, 3}; a refused pack
 * leaves w_packed untouched.  tsr_pack_conv_weight_bf16s writes nsplit * cout * cin * (padded taps) elements in the order
 * [cin/16][step][tap in step][plane][2][cout][8], plane p the bf16 of what the planes before it leave of the weight, padded
 * tap slots zero; tsr_conv_weight_bf16s_elems may be larger (never below nsplit * cout * round_up(cin, 32) * ks * ks) and the
 * pack leaves the surplus as it found it. */
long long tsr_conv_weight_bf16s_elems(int cout, int cin, int ks, int nsplit);   /* bf16 elements of w_packed */
int tsr_pack_conv_weight_bf16s(const float* w_oihw, void* w_packed, int cout, int cin, int ks, int nsplit,
                               void* stream);
int tsr_conv2d_fwd_bf16s(const float* in, int in_ctot, int in_coff, int cin,
                         const void* w_packed, int cout, int ks, int nsplit,
                         const float* scale, const float* shift,
                         const float* res, int res_ctot, int res_coff,
                         float* out, int out_ctot, int out_coff, int relu,
                         int B, int H, int W, void* stream);

/* The two stage-1 convolutions of an MSRB (3x3 64->64 and 5x5 64->64 on the same input,
 * model/tactileSR_model.py:167-175,198-200) as ONE launch on one staged halo (inference, fp16x3 arithmetic): a 5x5 conv
 * to 128 channels whose 3x3 half skips the 16 outer taps.  Output channels, scale and shift are in the kernel's channel
 * order: tsr_pair_channel_perm fills perm[k] = channel of torch.cat([conv3, conv5], 1) that kernel channel k holds; the
 * consumers' weights are permuted along C_in accordingly.  w_packed: tsr_conv_weight_pair_elems(cin) fp16 elements. */
int tsr_pair_channel_perm(int* perm128);      /* host array of 128 ints */
long long tsr_conv_weight_pair_elems(int cin);
int tsr_pack_conv_weight_pair_f16s(const float* w3_oihw, const float* w5_oihw, void* w_packed, int cin, float wscale,
                                   const float* w_amax, void* stream);
int tsr_conv2d_fwd_f16s_pair(const float* in, int in_ctot, int in_coff, int cin, const void* w_packed, float w_inv_scale,
                             const float* in_amax, float* out_amax, const float* scale, const float* shift,
                             float* out, int out_ctot, int out_coff, int relu, int B, int H, int W, void* stream);

/* fp16 two-plane variant ("fp16x3"): operands are scaled by powers of two into fp16's range -- weights at pack
 * time (wscale chosen by the caller: max|w|*wscale in [2^13,2^14); pass w_inv_scale = 1/wscale), activations in
 * the kernel from the device scalar in_amax = max|x| that the producer wrote through its out_amax -- then split
 * x*sx = h1+h2, w*sw = g1+g2 (22+ significand bits) and h1g1 + h1g2 + h2g1 are accumulated in fp32; the scales
 * are undone exactly in the epilogue.  Half the MFMA work of bf16x6; network-level error equal to the reference's
 * own fp32 CPU run against fp64 (tests).  Same remaining arguments as tsr_conv2d_fwd.
 *
 * in_amax / out_amax (the three fp16x3 inference launches: tsr_conv2d_fwd_f16s, _f16s_pair, _f16s_fuse1x1; checked launch by
 * launch in tests/test_gpu_infer_fp16x3.py):
 *  - in_amax (required) is an UPPER BOUND of max|x| over the input slice, not necessarily the maximum.  Only its exponent
 *    is used, sx = 2^(13 - floor(log2 in_amax)): two bounds of one binade give bit-identical results.  A bound 2^j times the
 *    true maximum costs at most j low bits of the activation planes: the error against fp64 stays below 2^j times the bar
 *    of the exact bound (measured for j = 1, 2: unchanged).  in_amax = 0 (an all-zero input) gives sx = 1 and exactly
 *    act(shift + res).
 *  - every scale is a power of two and is undone exactly: x * 2^k with in_amax * 2^k (power-of-two `scale`, no shift / res)
 *    gives exactly 2^k times the output and out_amax, as long as the input, the output and the factor the accumulator is
 *    multiplied by, w_inv_scale / sx = 2^(floor(log2 max|w|) + floor(log2 in_amax) - 26), stay normal fp32 numbers; sx itself
 *    is clamped to [2^-126, 2^127].  Held by the tests for |k| <= 60 on inputs of magnitude ~10.
 *  - out_amax (optional, NULL = off) follows the rule stated at tsr_stem_fwd: the slot is only ever RAISED by atomic max; the
 *    caller presets it (0, or the maximum so far -- two launches may share a slot), a prior above the launch's own maximum
 *    survives bit for bit, a prior below it ends as max|out| over the launch's output slice exactly.
 * Refusals (status 1, nothing is launched, `out` and `out_amax` are untouched) of the three launches: a NULL in, w_packed,
 * out or in_amax (fuse1x1: or w2_packed); B, H or W <= 0; cin <= 0; cin, any ctot or any coff not a multiple of 16; a negative
 * coff or a slice that leaves its buffer (coff + channels > ctot) for in, out and -- when res is given -- res; w_inv_scale
 * (fuse1x1: or w2_inv_scale) <= 0 or NaN; cout not in {64, 128}; ks not in {1, 3, 5} (fuse1x1: not in {3, 5}).  scale, shift,
 * res, shift2 and out_amax may each be NULL on their own (1 / 0 / no residual / 0 / off).  The pack routines refuse a NULL
 * weight or w_packed (_dev: or w_amax), cin <= 0 or not a multiple of 16, cout not in {64, 128}, ks not in {1, 3, 5} and a
 * wscale <= 0 or NaN (tsr_pack_conv_weight_pair_f16s: only when w_amax is NULL, which otherwise replaces wscale). */
int tsr_pack_conv_weight_f16s(const float* w_oihw, void* w_packed, int cout, int cin, int ks, float wscale,
                              void* stream);
/* Same with the scale derived ON THE DEVICE from w_amax[0] = max|w| (a device scalar the caller computed without a host
 * round trip): wscale = 2^(13 - floor(log2 max|w|)).  The matching convolution takes the same scalar through
 * tsr_conv_desc.w_amax. */
int tsr_pack_conv_weight_f16s_dev(const float* w_oihw, void* w_packed, int cout, int cin, int ks, const float* w_amax,
                                  void* stream);
int tsr_conv2d_fwd_f16s(const float* in, int in_ctot, int in_coff, int cin,
                        const void* w_packed, int cout, int ks, float w_inv_scale,
                        const float* in_amax, float* out_amax,
                        const float* scale, const float* shift,
                        const float* res, int res_ctot, int res_coff,
                        float* out, int out_ctot, int out_coff, int relu,
                        int B, int H, int W, void* stream);
/* MSRB stage-2 convolution with its half of the 1x1 `confusion` conv fused (model/tactileSR_model.py:196-206; no
 * `cat2` tensor in HBM).  W_c = [W_a | W_b]:  P = W_a.relu(bn(conv3(x1))) + b_c + x  (3x3 launch: w2 = W_a, shift2 = b_c,
 * res = x, relu2 = 0), out = relu(W_b.relu(bn(conv5(x1))) + P)  (5x5 launch: w2 = W_b, res = P, relu2 = 1).
 * fp16x3 arithmetic; the conv has C_out = 128; w2_packed = tsr_pack_conv_weight_f16s of the 64x128x1x1 half;
 * `out` / `res` / `out_amax` describe the 64-channel result. */
int tsr_conv2d_fwd_f16s_fuse1x1(const float* in, int in_ctot, int in_coff, int cin,
                                const void* w_packed, int ks, float w_inv_scale,
                                const float* in_amax, float* out_amax,
                                const float* scale, const float* shift, int relu,
                                const void* w2_packed, float w2_inv_scale, const float* shift2,
                                const float* res, int res_ctot, int res_coff,
                                float* out, int out_ctot, int out_coff, int relu2,
                                int B, int H, int W, void* stream);
/* bf16 ACTIVATION STORAGE (BASELINE's "bf16" configurations: reduced precision, tolerance 2e-2, never the parity path).
 * Activations are bf16 CB16 tensors -- `in` / `res` / `out` address bf16 elements, same [B][C/16][H*W][16] order --
 * weights the one-plane pack of tsr_pack_conv_weight_bf16s(nsplit = 1), fp32 accumulation and epilogue arithmetic
 * (same y = relu(conv*scale + shift + res) as tsr_conv2d_fwd).  tsr_stem_fwd_b16 writes such a tensor, tsr_head_fwd_b16
 * reads one (both otherwise identical to tsr_stem_fwd / tsr_head_fwd). */
int tsr_conv2d_fwd_b16(const void* in, int in_ctot, int in_coff, int cin, const void* w_packed, int cout, int ks,
                       const float* scale, const float* shift, const void* res, int res_ctot, int res_coff,
                       void* out, int out_ctot, int out_coff, int relu, int B, int H, int W, void* stream);
/* The bf16-storage INFERENCE convolutions proper (csrc/conv_b16k.hip; 3x3 / 5x5, C_out 64 / 128, C_in a multiple of 32):
 * v_mfma_f32_16x16x32_bf16 with channels as rows -- the accumulators are in CB16 order (8-B bf16 stores, no transpose)
 * and, for the fused form, already the operand layout of the 1x1 product -- LDS-DMA halo rows into a circular row buffer
 * and an LDS-DMA weight ring.  tsr_conv2d_fwd_b16k: same arguments and semantics as tsr_conv2d_fwd_b16.
 * tsr_conv2d_fwd_b16k_fuse1x1: a stage-2 convolution of an MSRB (128 -> 128, folded BatchNorm, ReLU) with its half of the
 * 1x1 `confusion` applied to the tile as it sits in the accumulator registers (see tsr_conv2d_fwd_f16s_fuse1x1; res / out
 * are 64-channel bf16 tensors).  tsr_conv2d_fwd_b16k_pair: the stage-1 pair of an MSRB, conv_3_1 || conv_5_1 (each conv +
 * BN + ReLU, model/tactileSR_model.py:167-175) and the first torch.cat (:200) as ONE launch on one staged halo: w_packed =
 * tsr_pack_conv_weight_b16k_pair(W = cat([3x3 weight zero-padded to 5x5, 5x5 weight]) along C_out, [128][cin][5][5];
 * tsr_conv_weight_b16k_pair_elems(cin) elements: one slab per barrier step, two outer taps per step), scale / shift = the two
 * convs' folded BatchNorm vectors concatenated (128), out = 128 channels in torch.cat order; the 3x3 half's MFMAs, fragment
 * reads and weight bytes on the 16 outer taps are skipped.  The weight layouts:
 * w_packed from tsr_pack_conv_weight_b16k ([C_in/32][tap][4][C_out][8] bf16; tsr_conv_weight_b16k_elems elements),
 * w2_packed from tsr_pack_w2_b16k (the 64x128 fp32 half of `confusion`, model/tactileSR_model.py:203-206, HALVED, in the K
 * order of the fused epilogue).
 * Refusals (status 1, nothing is launched, `out` is untouched) of tsr_conv2d_fwd_b16 and the three b16k launches (checked
 * launch by launch in tests/test_gpu_infer_b16.py, without a device in tests/test_infer_b16_cpu.py): a NULL in, w_packed or
 * out (fuse1x1: or w2_packed); B, H or W <= 0; cin <= 0; cin, any ctot or any coff not a multiple of 16 (the b16k forms: cin
 * not a multiple of 32); a negative coff or a slice that leaves its buffer (coff + channels > ctot) for in, out and -- when
 * res is given -- res; cout not in {64, 128}; ks not in {1, 3, 5} for tsr_conv2d_fwd_b16, not in {3, 5} for the b16k forms;
 * the b16k forms: 8 * in_ctot * H * W >= 2^31 (32-bit halo offsets inside a 4-image group).  scale, shift, res and shift2
 * may each be NULL on their own (1 / 0 / no residual / 0).  tsr_pack_conv_weight_b16k refuses a NULL pointer, cout not in
 * {64, 128}, cin <= 0 or not a multiple of 32 and ks not in {3, 5} (ks = 1: cout = 64 only); _b16k_pair a NULL pointer and
 * cin <= 0 or not a multiple of 32; tsr_pack_w2_b16k a NULL pointer.  tsr_conv_weight_b16k_elems = cout * cin * ks * ks,
 * tsr_conv_weight_b16k_pair_elems = (cin / 32) * 17 * 4096. */
long long tsr_conv_weight_b16k_elems(int cout, int cin, int ks);
int tsr_pack_conv_weight_b16k(const float* w_oihw, void* w_packed, int cout, int cin, int ks, void* stream);
int tsr_pack_w2_b16k(const float* w2_64x128, void* w_packed, void* stream);
/* Training with bf16 activation storage: a dgrad launch of tsr_conv2d_ex whose shape tsr_conv2d_ex_dgrad_b16k(nprime, cout,
 * ks) accepts may be described with nsplit = -3 instead of -1: it then runs on the same kernel (epi_mode 2, or 0 for the
 * unmasked partial gradient; no input / residual transform), with its weight packed by tsr_pack_conv_weight_dgrad_b16k
 * (arguments as tsr_pack_conv_weight_dgrad_bf16s, nprime = 128 or 64; tsr_conv_weight_b16k_elems(nprime, cout, ks) elements).
 * Slab entries as for nsplit = -1 (tsr_conv2d_slab_entries_ex accepts -3 / -4).  The predicate also accepts (128, 64, 1): the
 * masked dgrad of a 1x1 conv with 64 output channels (epi_mode 2, no partial gradient) as a streaming kernel without LDS
 * (csrc/conv1x1_b16k.hip; one slab entry per workgroup: ask tsr_conv2d_slab_entries_ex with nsplit = -3).  The same nsplit = -3 runs the FORWARD launches of that shape class (C_out = 64 or 128,
 * C_in a multiple of 32, 3x3 / 5x5, plain input: the predicate called as (cout, cin, ks)) there too: epi_mode 1 (raw output + Welford partials; weights from
 * tsr_pack_conv_weight_b16k) and epi_mode 0 with that pack; nsplit = -4 is epi_mode 1 of the stage-1 pair of an MSRB
 * (conv_3_1 || conv_5_1 as one 5x5 launch with 128 output channels, weights from tsr_pack_conv_weight_b16k_pair). */
int tsr_conv2d_ex_dgrad_b16k(int nprime, int cout, int ks);
/* 1 if tsr_conv2d_ex accepts nsplit = -3 for the FORWARD of a 1x1 conv of this shape whose input is VIRTUAL (in_scale /
 * in_shift set: relu(z * scale + shift) of the stored pre-BatchNorm tensor, formed in LDS behind the DMA): epi_mode 0 (shift =
 * bias, residual, ReLU), weights from tsr_pack_conv_weight_b16k(.., ks = 1).  csrc/conv1x1_b16k.hip. */
int tsr_conv2d_ex_fwd1x1_b16k(int cout, int cin);
int tsr_pack_conv_weight_dgrad_b16k(const float* w_oihw, void* w_packed, int cout, int cin, int ks, int ci0, int nprime,
                                    void* stream);
long long tsr_conv_weight_b16k_pair_elems(int cin);
int tsr_pack_conv_weight_b16k_pair(const float* w128_oihw5, void* w_packed, int cin, void* stream);
int tsr_conv2d_fwd_b16k(const void* in, int in_ctot, int in_coff, int cin, const void* w_packed, int cout, int ks,
                        const float* scale, const float* shift, const void* res, int res_ctot, int res_coff,
                        void* out, int out_ctot, int out_coff, int relu, int B, int H, int W, void* stream);
int tsr_conv2d_fwd_b16k_fuse1x1(const void* in, int in_ctot, int in_coff, int cin, const void* w_packed, int ks,
                                const float* scale, const float* shift, int relu,
                                const void* w2_packed, const float* shift2,
                                const void* res, int res_ctot, int res_coff,
                                void* out, int out_ctot, int out_coff, int relu2,
                                int B, int H, int W, void* stream);
int tsr_conv2d_fwd_b16k_pair(const void* in, int in_ctot, int in_coff, int cin, const void* w_packed,
                             const float* scale, const float* shift, void* out, int out_ctot, int out_coff,
                             int relu, int B, int H, int W, void* stream);
int tsr_stem_fwd_b16(const float* lr, int lr_ctot, int lr_coff, int axis_cnt, int hin, int win, int sf,
                     const float* w_oihw, const float* scale, const float* shift,
                     void* out_bf16, int out_ctot, int out_coff, int relu, int B, void* stream);
int tsr_head_fwd_b16(const void* in_bf16, int in_ctot, int cin, const float* w_oihw, float* out_nchw,
                     int relu, int B, int H, int W, void* stream);

/* nn.Upsample(scale_factor=sf, bilinear, align_corners=False) + Conv2d(3->64, 3x3, pad 1, no bias)
 * + scale/shift + optional ReLU: the pattern stem's first conv (model/tactileSR_model.py:34-39)
 * and the force stem (:59-63).  lr is the NCHW taxel tensor (B, lr_ctot, hin, win); channels
 * [lr_coff, lr_coff+3) are read (the x[:, 3t:3t+3] slices of :71-78).  Output CB16, H = hin*sf, W = win*sf.
 * hin and win are free (any taxel grid >= 1 x 1, a one-row image included); axis_cnt must be 3; scale and shift may be NULL
 * independently (1 and 0).  Images are cut into row bands so that one band (+ halo) of the upsampled image fits in LDS;
 * status 1 only when a band of two rows -- four padded rows of 3 x (((W + 3) & ~3) + 2) floats plus the taxels -- exceeds
 * 32 KB: W > 676 on 4 x 4 and on 1 x 4 taxels, i.e. sf > 169 (no TactileSR shape).  Every other bad argument (a NULL tensor, B, hin, win
 * or sf <= 0, out_ctot or out_coff not a multiple of 16, a slice that leaves [0, out_ctot) or [0, lr_ctot)) is status 1 too;
 * a refused call launches nothing. */
int tsr_stem_fwd(const float* lr, int lr_ctot, int lr_coff, int axis_cnt, int hin, int win, int sf,
                 const float* w_oihw, const float* scale, const float* shift,
                 float* out, int out_ctot, int out_coff, int relu, int B, float* out_amax, void* stream);
/* out_amax (optional device scalar): receives max|output| over the finite outputs (after the affine and the ReLU; NaN
 * outputs are skipped, a wave that holds an Inf publishes nothing) by atomic max -- the fp16-split convolution that
 * consumes the tensor derives its power-of-two input scale from it.  The slot is only ever RAISED: the caller presets it
 * (0, or the maximum so far), a value above the launch's own maximum is left as it was. */

/* Conv2d(cin->1, 3x3, pad 1, no bias) + ReLU, CB16 in, NCHW (B,1,H,W) out: output_layer[2:]
 * (model/tactileSR_model.py:55-56).  The trailing same-size F.interpolate (:83) is an identity.  Channels [0, cin) of the
 * in_ctot-channel input are read; cin and in_ctot multiples of 16, B, H, W > 0 (tsr_head_fwd_b16 alike): anything else is
 * status 1 before any launch. */
int tsr_head_fwd(const float* in, int in_ctot, int cin, const float* w_oihw, float* out_nchw,
                 int relu, int B, int H, int W, void* stream);

/* ---------------------------------------------------------------------------------------
 * Training path (train/tactileSR_train.py:41-51 -> cpu/trainer.py:346-362): train-mode
 * BatchNorm, convolution_backward (dgrad = tsr_conv2d_ex with tsr_pack_conv_weight_dgrad
 * weights, wgrad = tsr_conv2d_wgrad), MSE, Adam.
 * ------------------------------------------------------------------------------------- */

/* Extended convolution launch descriptor (plain C, device pointers; NULL/0 = unused).
 *  - in_scale/in_shift [cin]: x' = relu(x*s+t) applied to in-bounds input pixels while staging
 *    (the producer stored its raw bias-free conv output; its train-mode BN+ReLU happens here);
 *    res_scale/res_shift [cout]: same on the residual operand;
 *  - epi_mode 0: out = act(acc*scale+shift (+res));
 *    epi_mode 1: out = acc (raw); slab[(e*cout+c)*2+{0,1}] = (mean, M2) of the 64 pixels of entry
 *                e = (workgroup, image), slab_cnt[e] = valid pixel count  (BatchNorm batch statistics;
 *                entries = tsr_conv2d_slab_entries(B,H,W));
 *    epi_mode 2: out = (acc*scale (+res)) * [mask*mask_scale+mask_shift > 0]  (ReLU backward by the stored
 *                forward tensor `mask`); if bn_a: slab[(e*cout+c)*2+{0,1}] = (sum out, sum out*xhat),
 *                xhat = mask*bn_a+bn_b  (the two reductions of BatchNorm backward). */
typedef struct tsr_conv_desc {
  const float* in; int in_ctot; int in_coff; int cin;
  const float* w_packed; int cout; int ks;
  const float* scale; const float* shift;
  const float* res; int res_ctot; int res_coff;
  float* out; int out_ctot; int out_coff; int relu;
  int B; int H; int W;
  const float* in_scale; const float* in_shift;
  const float* res_scale; const float* res_shift;
  int epi_mode;
  const float* mask; int mask_ctot; int mask_coff;
  const float* mask_scale; const float* mask_shift;
  const float* bn_a; const float* bn_b;
  float* slab; float* slab_cnt;
  int nsplit;   /* -3 / -4: as -1 on csrc/conv_b16k.hip (see tsr_conv2d_ex_dgrad_b16k); -1: plain bf16 operands AND bf16 CB16 tensors (in / res / mask / out address bf16 elements; w_packed as
                   for 1): the train step with bf16 activation storage;
                   0: fp32 MFMA, w_packed from tsr_pack_conv_weight[_dgrad]; 1..3: split-bf16 MFMA (3 = fp32-equivalent),
                   w_packed from tsr_pack_conv_weight[_dgrad]_bf16s; -2: fp16 two-plane split ("fp16x3"), w_packed from
                   tsr_pack_conv_weight[_dgrad]_f16s, needs in_amax and w_inv_scale below */
  const float* in_amax;   /* device scalar max|in| (of the raw tensor; a fused input transform is bounded in-kernel) */
  float w_inv_scale;      /* 1 / wscale used at pack time */
  float* out_amax;        /* device scalar receiving max|out| (atomic max), any mode; NULL = off */
  const float* w_amax;    /* nsplit == -2, optional: device scalar max|w| of a weight packed by ..._f16s_dev; replaces
                             w_inv_scale (no host round trip for the weight scale) */
} tsr_conv_desc;

/* Refusals of tsr_conv2d_ex (status 1, nothing is launched; out, slab, slab_cnt and out_amax are untouched; checked launch by
 * launch in tests/test_gpu_conv_ex_b16k.py, without a device in tests/test_conv_ex_cases_cpu.py -- the table is
 * tests/_conv_ex_cases.py).  Every nsplit: desc = NULL; a NULL in, w_packed or out; B, H, W or cin <= 0; cin, any ctot or any
 * coff not a multiple of 16; a negative coff or a slice that leaves its buffer (coff + channels > ctot) for in, out, res (when
 * given) and mask (epi_mode 2); cout not in {64, 128}; ks not in {1, 3, 5}; epi_mode outside 0..2; epi_mode 1 without slab or
 * without slab_cnt; epi_mode 2 without mask; bn_a without bn_b or without slab (epi_mode 2; bn_a is read in no other mode); in_scale
 * without in_shift or the reverse, res_scale without res_shift or the reverse; nsplit outside -4..3.
 *   -2: a NULL in_amax; w_amax NULL and w_inv_scale not > 0 (0, negative, NaN).
 *   -1: the streaming 1x1 form (ks 1, C_out 64, epi_mode 0) keeps the whole weight in LDS: cin * 136 bytes > 72 KB (cin >= 544).
 *   -3, ks in {3, 5}: C_in not a multiple of 32 (48, 16); a virtual input (in_scale) or a virtual residual (res_scale);
 *       8 * in_ctot * H * W >= 2^31 (32-bit halo offsets inside a 4-image group); epi_mode 1 / 2 as above.
 *   -3, ks = 1: only two forms exist.  epi_mode 0 = the forward on a VIRTUAL input: refused with a plain input, with scale, with
 *       C_out != 64 or C_in not in {128, 256}, or 2 * in_ctot * H * W >= 2^31.  epi_mode 2 = the masked dgrad with N = cout = 128 and
 *       K = cin = 64: refused with res, scale, shift or an input transform, with N = 64 or K = 128, beyond the offset bound above.  epi_mode 1: always.
 *   -4: anything but ks 5, cout 128, epi_mode 1 with slab and slab_cnt, a plain input and C_in a multiple of 32 (ks 3, cout 64,
 *       epi_mode 0 or 2, no slab, a virtual input, C_in 48); the -3 offset bound. */
int tsr_conv2d_ex(const tsr_conv_desc* desc, void* stream);
int tsr_conv2d_slab_entries(int B, int H, int W);
/* Entries the launch described by (cout, ks, nsplit) writes -- the count to hand to tsr_bn_stats_finalize /
 * tsr_bn_bwd_finalize: ceil(B / img) * tiles * img, tiles = ceil(H / 8) * ceil(W / 8), img = images per workgroup of the
 * kernel that runs the launch -- 4 for the 3x3 / 5x5 launches of nsplit = -2 (fp16x3, both output widths) and of the
 * one-plane bf16 forms (nsplit = 1, -1, and -3 / -4), 2 for every other form: tsr_conv2d_slab_entries is the 2-image count.
 * Entry e = (image group * tiles + tile) * img + slot holds image group * img + slot; the slots of images >= B are written
 * with count 0 (epi_mode 1) / zero sums (epi_mode 2).  Size slabs for the larger of the two. */
int tsr_conv2d_slab_entries_ex(int B, int H, int W, int cout, int ks, int nsplit);

/* Weights of the data-gradient convolution: W'[n][co][kh][kw] = W[co][ci0+n][K-1-kh][K-1-kw],
 * n in [0,nprime), nprime in {64,128}; packed for tsr_conv2d_* with cin := cout, cout := nprime. */
int tsr_pack_conv_weight_dgrad(const float* w_oihw, float* w_packed, int cout, int cin, int ks,
                               int ci0, int nprime, void* stream);

int tsr_pack_conv_weight_dgrad_bf16s(const float* w_oihw, void* w_packed, int cout, int cin, int ks,
                                     int ci0, int nprime, int nsplit, void* stream);

int tsr_pack_conv_weight_dgrad_f16s(const float* w_oihw, void* w_packed, int cout, int cin, int ks,
                                    int ci0, int nprime, float wscale, void* stream);
int tsr_pack_conv_weight_dgrad_f16s_dev(const float* w_oihw, void* w_packed, int cout, int cin, int ks,
                                        int ci0, int nprime, const float* w_amax, void* stream);

/* Weight (and bias) gradient partials: slab[s][cout][cin][k][k] (s < nsplit, OIHW) with
 * dW = sum_s slab[s] (tsr_reduce_splits), from a = conv input (CB16, optional relu(a*scale+shift)
 * transform) and dz = gradient w.r.t. the conv output (CB16).  cin, cout multiples of 64.
 * bias_slab[s][cout] (optional, NULL = no bias gradient) receives sum over pixels of dz.
 * Split s sums a contiguous range of ceil(items / nsplit) work items, items = (image, patch) pairs: 8 x 8 patches here, 4-row x
 * 8-column ones in tsr_conv2d_wgrad_bf16s.  Any nsplit >= 1 is valid: a split whose range is empty -- nsplit above the item
 * count, or a last split the rounded-up range leaves nothing for -- still WRITES its partial (and bias partial), as exact
 * zeros, so tsr_reduce_splits over all nsplit partials is always right and a slab needs no clearing.  Partials are
 * deterministic (fixed summation order, no float atomics).  A rejected call (status 1) launches nothing and leaves slab /
 * bias_slab untouched. */
int tsr_conv2d_wgrad(const float* a, int a_ctot, int a_coff, int cin,
                     const float* a_scale, const float* a_shift,
                     const float* dz, int dz_ctot, int dz_coff, int cout, int ks,
                     float* slab, float* bias_slab, int nsplit, int B, int H, int W, void* stream);
/* Same on the 16-bit matrix cores with split operands: planes = 3 -> three bf16 planes, six products
 * (fp32-equivalent; a_amax/dz_amax unused); planes = 1 -> plain bf16 operands (reduced precision: the "bf16"
 * configurations, never the parity path); planes = -2 -> two power-of-two-scaled fp16 planes, three products,
 * scales derived from the device scalars a_amax = max|a| (raw tensor) and dz_amax = max|dz|;
 * planes = -1 -> plain bf16 operands read from bf16 CB16 TENSORS (`a`, `dz` then address bf16 elements): the train step
 * with bf16 activation storage (BASELINE configs[2] / [4], "bf16"; reference switch: cpu/trainer.py:96,203,346-362). */
int tsr_conv2d_wgrad_bf16s(const float* a, int a_ctot, int a_coff, int cin,
                           const float* a_scale, const float* a_shift,
                           const float* dz, int dz_ctot, int dz_coff, int cout, int ks, int planes,
                           const float* a_amax, const float* dz_amax,
                           float* slab, float* bias_slab, int nsplit, int B, int H, int W, void* stream);
/* Batch splits to launch tsr_conv2d_wgrad_bf16s with (slab / bias_slab hold that many partials): one resident round
 * of workgroups for this layer shape, never more than there are (image, 4x8 patch) work items; and the number of
 * workgroups one split launches (grid / nsplit of the launch: kernel-row groups x C_out tiles x C_in tiles of the tile the
 * launcher picks for (cout, cin, ks, planes)).  splits = clamp(slots / wgs_per_split, 1, B * ceil(H/4) * ceil(W/8)) with
 * slots = 256 for the 8-wave tiles and 512 for the 4-wave ones.  Both are host arithmetic, defined for the shapes
 * tsr_conv2d_wgrad_bf16s accepts (cout, cin multiples of 64; ks 1 / 3 / 5; planes 3 / 1 / -2 / -1). */
int tsr_conv2d_wgrad_splits(int cout, int cin, int ks, int planes, int B, int H, int W);
int tsr_conv2d_wgrad_wgs_per_split(int cout, int cin, int ks, int planes);
int tsr_reduce_splits(const float* slab, float* out, long long n, int nsplit, float alpha, void* stream);

/* nn.BatchNorm2d train mode (model/tactileSR_model.py:38,42,48,169,175,181,187), from the
 * epi_mode-1 slabs: batch mean / biased variance -> scale = gamma*invstd, shift = beta-mean*scale
 * (to apply on the bias-free conv output), xhat_a = invstd, xhat_b = -mean*invstd; running_mean/var
 * updated in place (momentum, unbiased variance, +bias on the mean).  work: 512*C*3 doubles. */
int tsr_bn_stats_finalize(const float* slab, const float* slab_cnt, int entries, int C,
                          const float* bias, const float* gamma, const float* beta,
                          float* running_mean, float* running_var, float momentum, float eps,
                          float* scale, float* shift, float* xhat_a, float* xhat_b,
                          double* work, void* stream);
/* Same statistics slabs for a 64-channel CB16 slice produced by a kernel without a stats epilogue
 * (the VALU stem): entries = tsr_cb16_stats_entries(B, HW). */
int tsr_cb16_stats_entries(int B, int HW);
int tsr_cb16_stats(const float* z, int z_ctot, int z_coff, int B, int HW, float* slab, float* slab_cnt,
                   void* stream);
/* BatchNorm backward reductions from the epi_mode-2 slabs: dgamma, dbeta and the coefficients of
 * dz = c1*g + c2*z + c3 (N = B*H*W). */
int tsr_bn_bwd_finalize(const float* slab, int entries, int C, double N, const float* scale,
                        const float* xhat_a, const float* xhat_b, float* dgamma, float* dbeta,
                        float* c1, float* c2, float* c3, double* work, void* stream);
int tsr_bn_bwd_apply(float* g, int g_ctot, int g_coff, const float* z, int z_ctot, int z_coff,
                     const float* c1, const float* c2, const float* c3, int C, int B, int HW,
                     float* out_amax /* optional: max|g| after the update */, void* stream);

/* nn.BatchNorm2d in EVAL mode inside a training module (`model.train()` then `bn.eval()` on some layers of
 * model/tactileSR_model.py:38,42,48,169-187: torch then normalises those layers with running_mean / running_var and leaves
 * the statistics alone).  tsr_bn_eval_vectors: the four forward vectors of tsr_bn_stats_finalize from the running
 * statistics, in double: invstd = 1/sqrt(running_var + eps), scale = gamma*invstd, shift = beta + (bias - running_mean)*scale,
 * xhat_a = invstd, xhat_b = (bias - running_mean)*invstd (to apply on the bias-free conv output; bias may be NULL).  One
 * launch, nothing is updated; C > 0 and a multiple of 16.
 * tsr_bn_bwd_finalize_eval: tsr_bn_bwd_finalize's slab reduction, emitting only dgamma = sum g*xhat and dbeta = sum g
 * (C = 64 or 128; work: 512*C*3 doubles).
 * tsr_bn_bwd_apply_eval: dz = scale * g, i.e. g[:, g_coff : g_coff + C] *= scale[c] in place on a CB16 tensor -- one read and
 * one write per element, no z (tsr_bn_bwd_apply moves three tensors).  C, g_ctot, g_coff multiples of 16, 0 <= g_coff,
 * g_coff + C <= g_ctot, B > 0, HW > 0; status 1 before any launch otherwise.  out_amax as for tsr_bn_bwd_apply. */
int tsr_bn_eval_vectors(const float* bias, const float* gamma, const float* beta, const float* running_mean,
                        const float* running_var, float eps, int C, float* scale, float* shift, float* xhat_a,
                        float* xhat_b, void* stream);
int tsr_bn_bwd_finalize_eval(const float* slab, int entries, int C, float* dgamma, float* dbeta, double* work,
                             void* stream);
int tsr_bn_bwd_apply_eval(float* g, int g_ctot, int g_coff, const float* scale, int C, int B, int HW,
                          float* out_amax /* optional: max|g| after the update */, void* stream);
/* (the bf16 CB16 form: fp32 product, one rounding on the store) */
int tsr_bn_bwd_apply_eval_b16(void* g, int g_ctot, int g_coff, const float* scale, int C, int B, int HW, void* stream);

/* Backward of tsr_stem_fwd's conv weight: slab[s][64][3][3][3] partials, s < nsplit, any nsplit >= 1 (the taxel gradient is
 * tsr_stem_dgrad).  Tall images are cut into row bands so that one band (+ halo) of the upsampled image fits in LDS: the
 * bands are spread over the splits as far as they divide nsplit, a workgroup walks the rest; status 1 only when three
 * padded rows of 3 x (W + 2) floats plus the taxels exceed 160 KB (no TactileSR shape). */
int tsr_stem_wgrad(const float* lr, int lr_ctot, int lr_coff, int hin, int win, int sf,
                   const float* dz, int dz_ctot, int dz_coff, float* slab, int nsplit, int B, void* stream);
/* Taxel gradient of the stem (reference model/tactileSR_model.py:35-37,60-61: Upsample(bilinear, align_corners=False) +
 * Conv2d(3 -> 64, 3x3, pad 1, no bias)): dx = up_sf^T(conv3x3^T(dz; w_oihw)) for the 64 CB16 channels
 * dz_coff .. dz_coff + 63 of dz (pre-BN / pre-ReLU-masked gradient).  dx is NCHW fp32 (B, dx_ctot, hin, win); channels
 * dx_coff .. dx_coff + 2 are stored (accumulate = 0) or added to (accumulate = 1).  hin, win <= 4; fp32 arithmetic, one
 * workgroup per image, bit-reproducible. */
int tsr_stem_dgrad(const float* w_oihw, const float* dz, int dz_ctot, int dz_coff, int hin, int win, int sf,
                   float* dx, int dx_ctot, int dx_coff, int accumulate, int B, void* stream);
/* Backward of tsr_head_fwd: dz_h0 = dgrad(dout*[out>0]) * [h0>0] (CB16) and weight partials
 * wslab[s][cin][3][3].  The weight gradient holds the zero-padded H x W image in 64 KB of LDS: (H + 2)(W + 2) <= 16384,
 * i.e. at most 126 x 126 -- TactileSR trains at scale_factor <= 31 on 4 x 4 taxels.  Larger shapes return 1 before any
 * launch (dz_h0, wslab and dz_amax untouched). */
int tsr_head_bwd(const float* dout, const float* out, const float* h0, int h_ctot, int cin,
                 const float* w_oihw, float* dz_h0, int dz_ctot, float* wslab, int nsplit,
                 int B, int H, int W, float* dz_amax /* optional: max|dz_h0| */, void* stream);
/* The activation-gradient half of tsr_head_bwd alone, for a train step whose 128 -> 1 head conv (reference
 * model/tactileSR_model.py:55-56: Conv2d(128, 1, 3, padding=1, bias=False) + ReLU) is frozen while layers below it still
 * train: dz_h0 = dgrad(dout*[out>0]) * [h0>0] and dz_amax are tsr_head_bwd's bit for bit (the same kernel launch), no weight
 * partials are formed.  tsr_head_bwd's argument checks without the wslab / nsplit ones and without the (H + 2)(W + 2) bound,
 * which is the weight gradient's; H * W <= 2^28. */
int tsr_head_dgrad(const float* dout, const float* out, const float* h0, int h_ctot, int cin,
                   const float* w_oihw, float* dz_h0, int dz_ctot, int B, int H, int W,
                   float* dz_amax /* optional: max|dz_h0| */, void* stream);

/* The same four kernels on bf16 CB16 tensors -- the train step with bf16 ACTIVATION STORAGE (tsr_conv_desc.nsplit = -1,
 * tsr_conv2d_wgrad_bf16s planes = -1): every stored activation / gradient tensor is bf16, arithmetic and the
 * statistics / weight-gradient slabs stay fp32.  Pointers typed void* address bf16 elements. */
int tsr_cb16_stats_b16(const void* z, int z_ctot, int z_coff, int B, int HW, float* slab, float* slab_cnt,
                       void* stream);
int tsr_bn_bwd_apply_b16(void* g, int g_ctot, int g_coff, const void* z, int z_ctot, int z_coff,
                         const float* c1, const float* c2, const float* c3, int C, int B, int HW, void* stream);
/* tsr_stem_dgrad on a bf16 CB16 dz (fp32 arithmetic, fp32 dx). */
int tsr_stem_dgrad_b16(const float* w_oihw, const void* dz, int dz_ctot, int dz_coff, int hin, int win, int sf,
                       float* dx, int dx_ctot, int dx_coff, int accumulate, int B, void* stream);
/* out[B][C/16][HW][16] (bf16) = bf16(relu(fp32(z) * scale + shift)) of channels z_coff .. z_coff + C of the stored
 * pre-BatchNorm tensor: the MATERIALISED form of a virtual activation.  tsr_conv2d_wgrad_bf16s (planes = -1) runs the 3x3 /
 * 5x5 launches for which tsr_conv2d_wgrad_b16k(cout, cin, ks) returns 1 on csrc/wgrad_b16k.hip (operands straight from HBM
 * into LDS) when they carry NO input transform: a caller with a virtual input materialises it once and passes it plain. */
int tsr_bn_relu_b16(const void* z, int z_ctot, int z_coff, int C, const float* scale, const float* shift, void* out,
                    int B, int HW, void* stream);
int tsr_conv2d_wgrad_b16k(int cout, int cin, int ks);
int tsr_stem_wgrad_b16(const float* lr, int lr_ctot, int lr_coff, int hin, int win, int sf,
                       const void* dz, int dz_ctot, int dz_coff, float* slab, int nsplit, int B, void* stream);
int tsr_head_bwd_b16(const float* dout, const float* out, const void* h0, int h_ctot, int cin,
                     const float* w_oihw, void* dz_h0, int dz_ctot, float* wslab, int nsplit,
                     int B, int H, int W, void* stream);
/* tsr_head_dgrad on bf16 CB16 h0 / dz_h0 (reference model/tactileSR_model.py:55-56). */
int tsr_head_dgrad_b16(const float* dout, const float* out, const void* h0, int h_ctot, int cin,
                       const float* w_oihw, void* dz_h0, int dz_ctot, int B, int H, int W, void* stream);

/* HR.float()/HR_scale_num + F.interpolate(size=(H,W), bilinear) (train/tactileSR_train.py:44-45). */
int tsr_target_prep(const float* hr_raw, float* out, float inv_scale, int B, int hin, int win, int H, int W,
                    void* stream);
/* nn.MSELoss() forward (loss[0]) and backward (dy = grad_scale*2(y-t)/n; dy may be NULL).  work: 256 doubles. */
int tsr_mse_fwd_bwd(const float* y, const float* target, float* dy, float* loss, long long n,
                    float grad_scale, double* work, void* stream);
/* torch.optim.Adam step with L2-in-gradient weight decay (train/tactileSR_train.py:212); step is 1-based. */
int tsr_adam_l2_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n,
                     float lr, float beta1, float beta2, float eps, float weight_decay, int step, void* stream);
/* The same step for MANY tensors in one launch (the reference's optim.Adam over all 124 parameter tensors,
 * train/tactileSR_train.py:212; cpu/trainer.py:361): `chunks` is a DEVICE array of n_chunks records, one per
 * <= 4096-element piece of a tensor, pointers already offset to the piece.  The same formula as tsr_adam_l2_step, not the
 * same bits: the two kernels are compiled separately and the multiply-adds of the moment updates are fused in one and not
 * in the other, so exp_avg, exp_avg_sq and the parameter can differ in the last bit between the two forms. */
typedef struct tsr_adam_chunk {
  float* param; const float* grad; float* exp_avg; float* exp_avg_sq;
  int n; int reserved;
} tsr_adam_chunk;
int tsr_adam_l2_multi(const tsr_adam_chunk* chunks, int n_chunks, float lr, double beta1, double beta2, float eps,
                      float weight_decay, int step, void* stream);
/* The per-step scalars of tsr_adam_l2_multi, {lr, bc1, bc2_sqrt} = {lr, 1 - beta1^step, sqrt(1 - beta2^step)} formed in
 * double and rounded to float (cpu/trainer.py:361: optimizer.step()'s bias corrections), written to the HOST array out3:
 * the values the plain launch passes for the same arguments, bit for bit.  Host-only; step is 1-based. */
int tsr_adam_hyper(float lr, double beta1, double beta2, int step, float* out3);
/* tsr_adam_l2_multi with its per-step scalars read from the DEVICE array hyper = {lr, bc1, bc2_sqrt} (filled through
 * tsr_adam_hyper) instead of kernel arguments, so a captured graph replays the step of cpu/trainer.py:361 with the lr
 * and bias corrections of each replay.  Same kernel body, same arithmetic. */
int tsr_adam_l2_multi_dev(const tsr_adam_chunk* chunks, int n_chunks, const float* hyper, double beta1, double beta2,
                          float eps, float weight_decay, void* stream);
/* Gradient-norm clipping (cpu/trainer.py:354-356: clip_grad_norm_(model.parameters(), max_norm) before the step).
 * tsr_grad_norm_multi: the global L2 norm of the GRADIENTS the chunk records point at (chunk.grad, chunk.n; the other
 * fields are not read) and torch's clip coefficient, written to the DEVICE array out2 = {total_norm, clip_coef}.
 * Two launches, deterministic (no float atomics): a fixed grid of 256 workgroups writes one double partial each into
 * work (>= 256 doubles), squaring and summing within a chunk in fp32; one workgroup sums the partials in a fixed order
 * in double; total_norm = (float)sqrt(sum).  clip_coef is torch's fp32 arithmetic bit for bit:
 * min((total_norm + 1e-6f).reciprocal() * max_norm, 1) with a clamp that keeps a NaN -- a NaN gradient gives a NaN
 * norm and coefficient, an Inf gradient an Inf norm and a coefficient of 0.  The norm can differ from torch's by a
 * few ulps (another summation order).  Edge case: because the partials are combined in double, a norm whose per-chunk
 * sums of squares stay finite in fp32 but whose total overflows fp32 comes out finite here, where torch returns Inf.
 * tsr_adam_l2_multi_clip / tsr_adam_l2_multi_dev_clip: tsr_adam_l2_multi / tsr_adam_l2_multi_dev on the clipped
 * gradient g' = g * clip[0] (one fp32 multiply, rounded on its own), clip a DEVICE pointer to the coefficient
 * (out2 + 1).  They WRITE g' back through chunk.grad (torch leaves p.grad clipped; skipped where clip[0] == 1, which
 * is exact).  Result: bit for bit "clip the gradient in fp32, then the plain step". */
int tsr_grad_norm_multi(const tsr_adam_chunk* chunks, int n_chunks, float max_norm, double* work, float* out2,
                        void* stream);
int tsr_adam_l2_multi_clip(const tsr_adam_chunk* chunks, int n_chunks, float lr, double beta1, double beta2, float eps,
                           float weight_decay, int step, const float* clip, void* stream);
int tsr_adam_l2_multi_dev_clip(const tsr_adam_chunk* chunks, int n_chunks, const float* hyper, double beta1,
                               double beta2, float eps, float weight_decay, const float* clip, void* stream);

/* The Adam family beyond the reference's choice, in the same one launch over a chunk table (csrc/adam_ex.hip):
 * decoupled weight decay (torch.optim.AdamW) and AMSGrad (amsgrad=True of either torch class).  `flags` is an OR of
 * the two bits below; flags = 0 is torch.optim.Adam's formula (tsr_adam_l2_multi's, from another kernel: the same
 * formula, not promised the same bits).  One workgroup of 256 threads per tsr_adam_chunk record; 16-byte accesses
 * when every pointer of the record (vmax's too, when it is used) is 16-byte aligned, scalar otherwise and for the tail.
 * `vmax` is a DEVICE array of n_chunks pointers, one per record, already offset to the piece like the record's own
 * pointers: torch's max_exp_avg_sq.  It is required with TSR_ADAM_AMSGRAD and must be NULL without it.
 * Per element, with b1/b2 = (float)beta, omb = (float)(1 - beta) formed in double, and hyper4 = {lr, bc1, bc2_sqrt, decay}:
 *   g      = clip ? g * clip[0] : g        one fp32 multiply, written back through chunk.grad unless clip[0] == 1
 *   L2:        gg = fmaf(wd, w, g);  w0 = w
 *   DECOUPLED: gg = g;               w0 = w * decay             (one fp32 multiply: torch's param.mul_(1 - lr * wd))
 *   m      = b1*m + omb1*gg ;  v = b2*v + omb2*gg*gg
 *   AMSGRAD:   vm = (v or vm is NaN) ? NaN : max(vm, v);  vhat = vm     (torch.maximum: a NaN propagates)
 *   else:      vhat = v
 *   p      = w0 - (lr/bc1) * (m / (sqrtf(vhat)/bc2_sqrt + eps))
 * Every fp32 operation above is rounded on its own (the fmaf is the only fused one), in every flag combination and on
 * both the 16-byte and the scalar path: with weight_decay = 0 the DECOUPLED and the L2 form give the same bits.
 * tsr_adam_hyper_ex writes hyper4 to the HOST array out4: the first three are tsr_adam_hyper's floats bit for bit,
 * decay = (float)(1.0 - (double)lr * (double)weight_decay) with TSR_ADAM_DECOUPLED and 1.0f without.
 * tsr_adam_multi_ex forms them on the host and passes them as kernel arguments; tsr_adam_multi_ex_dev reads them from
 * the DEVICE array hyper4, so a captured graph replays the step with the values written before that replay: same kernel
 * body, same bits for the same floats.  `clip` (NULL: no clipping) is a DEVICE pointer to the coefficient
 * tsr_grad_norm_multi wrote (out2 + 1).
 * Refused with TSR_ERR_ARG before any launch: chunks NULL; n_chunks <= 0; a flag bit outside the two defined;
 * TSR_ADAM_AMSGRAD without vmax, or vmax without it; step <= 0 (host-scalar form); hyper4 NULL (device form); out4
 * NULL; lr, eps or weight_decay NaN or negative; a beta outside [0, 1).  A record whose n is outside 1..4096 is skipped
 * by its workgroup: nothing is read or written through its pointers. */
#define TSR_ADAM_DECOUPLED 1
#define TSR_ADAM_AMSGRAD 2
int tsr_adam_hyper_ex(float lr, double beta1, double beta2, int step, float weight_decay, int flags, float* out4);
int tsr_adam_multi_ex(const tsr_adam_chunk* chunks, float* const* vmax, int n_chunks, int flags, float lr, double beta1,
                      double beta2, float eps, float weight_decay, int step, const float* clip, void* stream);
int tsr_adam_multi_ex_dev(const tsr_adam_chunk* chunks, float* const* vmax, int n_chunks, int flags,
                          const float* hyper4, double beta1, double beta2, float eps, float weight_decay,
                          const float* clip, void* stream);

/* Weight averaging (EMA / SWA) of every tensor of a state dict in ONE launch.  `chunks` is a DEVICE array of n_chunks
 * records, one per piece of 1..4096 4-byte words of a tensor, pointers already offset to the piece: avg is the average
 * (the shadow), src the live tensor.  One workgroup of 256 threads per record; 16-byte accesses when both pointers of
 * the record are 16-byte aligned, scalar otherwise (and for the tail).  mode 0 = fp32 values, mode 1 = raw words
 * (integer buffers such as num_batches_tracked, an int64 as two words per element, or a buffer to be copied).
 *   op 0 UPDATE  mode 0: avg = fmaf(omd, src - avg, avg), omd = one_minus_decay, the subtraction rounded in fp32
 *                        (|result - exact| <= 3 * 2^-24 * max(|src|, |avg|));  mode 1: avg = src.
 *   op 1 STORE   avg = src for every record (initialisation)
 *   op 2 LOAD    src = avg for every record
 *   op 3 SWAP    the two are exchanged for every record
 * STORE, LOAD, SWAP and mode 1 move raw words: bit for bit, NaN payloads and integers included; two SWAPs are the
 * identity on bits.  UPDATE consequences: src == avg (the same value, or a record naming the same words twice: a frozen
 * parameter) leaves a finite avg unchanged bit for bit (src - avg is +0; a -0 average becomes the equal +0, an Inf one
 * NaN, as Inf - Inf is); avg == 0 with omd == 1 gives src exactly; a NaN or Inf stays in its own element.  avg and src
 * of one record may be identical but must not overlap otherwise, and no two records may share a word.
 * tsr_ema_multi_dev reads omd from the DEVICE float one_minus_decay_dev instead of a kernel argument, so a captured
 * graph replays the launch with the value written before that replay (a decay that warms up); same kernel body, same
 * bits for the same float.  Its value is the caller's to keep in [0, 1].
 * Refused with TSR_ERR_ARG before any launch: chunks NULL, n_chunks <= 0, op outside 0..3, one_minus_decay NaN or
 * outside [0, 1], one_minus_decay_dev NULL.  A record whose n is outside 1..4096 or whose mode is outside 0..1 is
 * skipped by its workgroup: nothing is read or written through its pointers. */
typedef struct tsr_ema_chunk { float* avg; float* src; int n; int mode; } tsr_ema_chunk;
int tsr_ema_multi(const tsr_ema_chunk* chunks, int n_chunks, int op, float one_minus_decay, void* stream);
int tsr_ema_multi_dev(const tsr_ema_chunk* chunks, int n_chunks, int op, const float* one_minus_decay_dev,
                      void* stream);

/* Per-sample PSNR / SSIM of eval_func (train/tactileSR_train.py:87-94, utility/tools.py:49-81) for B samples
 * of n elements: PSNR = 10log10(max^2/(sum(a-b)^2/psnr_div)) with psnr_div = shape[0]*shape[1] of what the
 * reference passes ((1,H,W) -> H, its /40 quirk; (H,W) -> H*W); SSIM = one global window. */
int tsr_psnr_ssim(const float* a, const float* b, int B, int n, double psnr_div, double max_value,
                  double C1, double C2, float* psnr, float* ssim, void* stream);

/* Differentiable SSIM (utility/tools.py:66-81 calculationSSIM, :84-114 class SSIM "# ssim loss"): per-image SSIM of the
 * prediction y against the target t, both (B,1,H,W) NCHW fp32 contiguous, and its gradient with respect to y, from ONE
 * launch (csrc/ssim_loss.hip).
 *   win = 0          the global form: one window per image with weight 1/(H*W) -- calculationSSIM's formula, the
 *                    value tsr_psnr_ssim reports; H*W <= 2^28.
 *   win in 3,5,..11  the windowed form: the 1-D Gaussian g[k] ~ exp(-(k - (win-1)/2)^2 / (2 sigma^2)), normalised to
 *                    sum 1, applied separably as a VALID correlation G[.]; the map is (H-win+1) x (W-win+1);
 *                    win <= H, W <= 128.  sigma is not read when win = 0.
 * With x = y (the prediction):
 *   mx = G[x], mt = G[t], sxx = G[x^2] - mx^2, stt = G[t^2] - mt^2, sxt = G[x t] - mx mt
 *   A1 = 2 mx mt + C1, A2 = 2 sxt + C2, B1 = mx^2 + mt^2 + C1, B2 = sxx + stt + C2, S = A1 A2 / (B1 B2)
 *   ssim[b] = mean of S over image b's map (N positions)
 *   P = 2 mt (A2 - A1)/(B1 B2) - 2 mx S (1/B1 - 1/B2),  Q = -S/B2,  R = 2 A1/(B1 B2)
 *   d ssim[b] / d y_p = (1/N) (G^T[P] + 2 y_p G^T[Q] + t_p G^T[R]),  G^T the adjoint (full) correlation.
 * dy (optional; NULL = values only) (B,1,H,W):  dy = dy_scale * d ssim[b]/d y  when accumulate = 0,
 * dy += the same when accumulate = 1 (the train step folds the term into the MSE gradient this way).
 * All window sums, S, P, Q, R and the adjoint sums are fp64 (the moments cancel: fp32 misses 1e-5); values and gradients
 * are rounded to fp32 once, at the store.  One workgroup per image, fixed summation order, no atomics: two launches
 * give the same bits.  Images are independent: a NaN or Inf pixel makes its own image's ssim NaN and its gradient
 * NaN wherever a window holds the pixel (everywhere when win = 0), as in torch; every other image is untouched.
 * Refusals (status 1, nothing launched, ssim and dy untouched): a NULL y, t or ssim; B, H or W <= 0; win negative,
 * even, 1 or above 11; with win > 0, H or W below win or above 128, or sigma <= 0 or NaN; H*W > 2^28 with win = 0;
 * C1 or C2 <= 0 or NaN; accumulate not 0 or 1; dy_scale NaN. */
int tsr_ssim_fwd_bwd(const float* y, const float* t, int B, int H, int W, int win, double sigma, double C1, double C2,
                     float* ssim, float* dy, float dy_scale, int accumulate, void* stream);

/* Pixel losses of the train step (csrc/pixel_loss.hip): MSE, L1, Charbonnier and Huber of d = y - t over n fp32 elements,
 * with an optional contact weight, and the gradients with respect to the prediction y AND the target t from one pass.
 * d is the exact difference of the two floats, carried in double.
 *   kind 0  MSE          rho(d) = d^2                                                        param not read
 *   kind 1  L1           rho(d) = |d|                           rho'(0) = sign(0) = 0        param not read
 *   kind 2  Charbonnier  rho(d) = sqrt(d^2 + eps^2)                                          param = eps > 0
 *   kind 3  Huber        rho(d) = d^2/2 for |d| <= delta, else delta (|d| - delta/2)         param = delta > 0
 *                        (torch's HuberLoss; both branches agree at |d| = delta)
 *   w_p = 1 + fg_weight [t_p > fg_threshold]   the comparison on the fp32 values (exact); a NaN target compares false
 *   loss[0] = (1/n) sum_p w_p rho(d_p)         the divisor is n, not sum w: fg_weight = 0 is the unweighted loss, and a
 *                                              background pixel's gradient does not depend on the batch's contact count
 *   g_p = w_p rho'(d_p) / n
 * dy (optional) (n):  dy = dy_scale * g when accumulate = 0,  dy += dy_scale * g when accumulate = 1 -- the contract of
 * tsr_ssim_fwd_bwd, whose launch can keep accumulating behind this one.
 * dt (optional) (n), always overwritten:  dt = -dy_scale * g, the exact target gradient (every loss depends on y - t only,
 * and the weight is not differentiated).  dt and dy must not alias.
 * Summation: fp64 in a fixed order -- one partial per workgroup into work (TSR_PIXEL_LOSS_WORK doubles), then one small
 * launch that adds them in a fixed order; no floating-point atomics, no completion counter: two launches give the same
 * bits.  The value and every gradient element are computed in fp64 and rounded to fp32 once, at the store (an L1 element
 * is the fp32 rounding of +-dy_scale w / n, a linear Huber element that of +-dy_scale delta w / n).
 * A streaming kernel (grid-stride, at most TSR_PIXEL_LOSS_WORK workgroups): 16-byte loads and stores with a scalar head
 * and tail where y, t and the given dy, dt sit at one common offset from 16-byte alignment (any multiple of 4 bytes);
 * pointers at different offsets are served one float at a time.
 * Non-finite input: elements are independent.  A non-finite d_p reaches the loss and its own dy / dt element; every other
 * gradient element keeps the bits of the clean run.  A NaN d_p gives NaN in its element for every kind (for L1 unlike
 * torch, whose sign(NaN) is 0: a silent zero would hide a bad pixel).  d_p = +-Inf gives what the formula gives in IEEE
 * arithmetic: MSE +-Inf, L1 +-dy_scale w / n, Huber +-dy_scale delta w / n, Charbonnier NaN.  The loss is NaN if any d_p
 * is NaN, otherwise +Inf.
 * Refusals (status 1, nothing launched, nothing written): a NULL y, t, loss or work; n <= 0; kind outside 0..3; kind 2 or
 * 3 with param <= 0, NaN or Inf; fg_weight < 0, NaN or Inf; fg_threshold NaN; accumulate not 0 or 1; accumulate = 1 with
 * dy NULL; dy_scale NaN; dt == dy when both are given. */
#define TSR_PIXEL_LOSS_WORK 2048
int tsr_pixel_loss_fwd_bwd(const float* y, const float* t, long long n, int kind, double param, float fg_weight,
                           float fg_threshold, float* loss, float* dy, float dy_scale, int accumulate, float* dt,
                           double* work, void* stream);

/* Degradation-consistency loss (csrc/degrade_loss.hip): the sensor model's pooling of an image onto the 4x4 taxels
 * (reference model/tPSFNet.py:129-141, degradation_process: Gaussian masks around the taxel centres, scaled to (0, 1)),
 * generalised from the 100x100 grid to any H x W, the mean squared residual against measured taxels z, and its gradients
 * with respect to the image and to z, from one launch.  For image b with width gamma in (0, 1e6]:
 *   KM = 100/15138,  c_a = 12 + 25 a (a = 0..3),  mn = exp(-100/gamma)
 *   X(x) = (x + 0.5) 100/H - 0.5,  Y(v) = (v + 0.5) 100/W - 0.5     the pixel centres of F.interpolate(align_corners=False)
 *   E_a[x] = exp(-KM (X(x) - c_a)^2 / gamma),  F_c[v] = exp(-KM (Y(v) - c_c)^2 / gamma)
 *   k = gain 1e-4 (100/H)(100/W) / (1 - mn)
 *   D_ac = k (sum_xv E_a[x] y_xv F_c[v] - mn sum_xv y_xv)           lr_deg[b][4a + c]; H = W = 100, gain 1: the reference's
 *   r_ac = D_ac - z_ac,  q[b] = (1/16) sum_ac r_ac^2
 *   dq/dy_xv = (2/16) k (sum_ac r_ac E_a[x] F_c[v] - mn sum_ac r_ac),  dq/dz_ac = -(2/16) r_ac
 * The upper limit TSR_DEGRADE_GAMMA_MAX = 1e6 is where the operator stops meaning anything, well before it stops being
 * computable: as gamma grows every mask tends to the constant 1 and D to the difference of two nearly equal sums over a
 * vanishing 1 - mn (from about 1e18 on 1 - mn rounds to 0 and k is Inf).  At 1e6 the masks vary by 1e-4 over the sensor,
 * far flatter than any width the sensor model is trained to (a few tens at most), and 1 - mn still carries twelve digits.
 * gamma is not differentiated.  gain undoes a scaling of the image (the train step's target is HR / HR_scale_num).
 * y (B,1,H,W) fp32 contiguous, 1 <= H, W <= 128.  z: taxel (a,c) of image b at z[b z_bstride + 4a + c], so a channel slice
 * of a (B,C,4,4) tensor is passed in place; NULL = the forward alone (q, dy, dz must then be NULL and lr_deg given).
 * gamma_dev (B) on the device, NULL = gamma_all for every image; where gamma_dev[b] == gamma_all the bits are those of the
 * NULL form.  lr_deg (B,16) optional.  q (B), required with z.  dy (B,1,H,W) optional, the contract of tsr_ssim_fwd_bwd:
 * dy = dy_scale dq/dy when accumulate = 0, dy += the same when accumulate = 1; it must not overlap y.  dz (B,16) optional,
 * always overwritten with dy_scale dq/dz.
 * Arithmetic: the tables, every sum, r and the gradients are fp64 from the exact fp32 inputs; a value is rounded to fp32
 * once, at its store.  One workgroup per image, at most TSR_DEGRADE_MAX_WGS of them walking the batch; the 16 + 1 sums are
 * reduced in a fixed order and there are no atomics: two launches give the same bits.  The image is read once (the gradient
 * needs r and the tables only).  float4 loads when W % 4 == 0 and y is 16-byte aligned, float4 stores when W % 4 == 0 and dy
 * is; otherwise the same four columns move one float at a time through the same arithmetic, with the same bits.
 * Non-finite input: images are independent.  A NaN or Inf pixel makes its own image's lr_deg, q and whole dy non-finite
 * (the mn sum y term reaches every taxel).  A device gamma that is <= 0, NaN or above 1e6 (Inf included) makes that image's lr_deg, q, dz and dy
 * all-NaN (dy whatever accumulate says), never an out-of-range access.  Every other image keeps the bits of the clean run.
 * Refusals (status 1, before any device call, nothing written): a NULL y; B, H or W <= 0; H or W > 128; gamma_dev NULL with
 * gamma_all <= 0, NaN or above 1e6 (Inf included); gain NaN or Inf; z without q; z NULL with q, dy or dz given or without lr_deg; z_bstride < 16
 * with B > 1; accumulate not 0 or 1; accumulate = 1 without dy; dy_scale NaN; dy overlapping y. */
#define TSR_DEGRADE_MAX_WGS 2048
#define TSR_DEGRADE_GAMMA_MAX 1e6
int tsr_degrade_fwd_bwd(const float* y, int B, int H, int W, const float* z, long long z_bstride, const float* gamma_dev,
                        double gamma_all, double gain, float* lr_deg, float* q, float* dy, float dy_scale, int accumulate,
                        float* dz, void* stream);
/* The same launch with the caller's grid cap (tsr_degrade_fwd_bwd is this with max_wgs = TSR_DEGRADE_MAX_WGS): at most
 * max_wgs workgroups, each walking the further images at a stride of the grid.  The result does not depend on max_wgs,
 * bit for bit.  Refusals: those above, and max_wgs < 1. */
int tsr_degrade_fwd_bwd_wgs(const float* y, int B, int H, int W, const float* z, long long z_bstride,
                            const float* gamma_dev, double gamma_all, double gain, float* lr_deg, float* q, float* dy,
                            float dy_scale, int accumulate, float* dz, int max_wgs, void* stream);

/* Per-sample supervision weights (csrc/sample_weight.hip, csrc/pixel_loss.hip, csrc/ssim_loss.hip): every image b of a
 * batch of B carries a weight w_b >= 0 with which the pixel and SSIM terms count it; w_b = 0 is an unlabeled image whose
 * target is never read.  With P = H W pixels per image, omega_p = 1 + fg_weight [t_p > fg_threshold], rho and d_p as in
 * tsr_pixel_loss_fwd_bwd, ssim_b as in tsr_ssim_fwd_bwd and q_b as in tsr_degrade_fwd_bwd (which takes no weight):
 *   pix_b = (1/P) sum_p omega_p rho(d_p)
 *   L     = (1/B) sum_{s_b != 0} s_b [pix_b + ls (1 - ssim_b)]  +  ld (1/B) sum_b q_b
 *   dL/dy_bp = (s_b/B) [omega_p rho'(d_p)/P - ls d ssim_b/d y_bp]  +  (ld/B) d q_b/d y_bp
 * A weight is VALID when it is finite and >= 0 (-0 is 0).  The scale s_b of tsr_sample_scale:
 *   mode 0 ("sum")    D = sum of the valid w_b, fp64, in index order;  s_b = fl32(w_b B / D), or 0 when D == 0: the
 *                     supervised terms are means over the labeled weight; uniform weights give s_b = 1 exactly
 *   mode 1 ("batch")  s_b = w_b: the divisor stays B
 *   an invalid w_b    s_b = NaN, and w_b is left out of D: that image's terms are NaN, no other image's are
 * stats[0] = fl32(D), stats[1] = the number of valid w_b > 0 (both modes).  One workgroup.  s must not alias w.
 * A SKIPPED image is one whose s_b == 0 exactly: its y and t are not read, its entry of a value vector (pix, ssim) is
 * written as 0, its dy rows are 0 on overwrite and untouched on accumulate, its dt rows are 0.
 *
 * tsr_pixel_loss_ps_fwd_bwd is the per-image form of tsr_pixel_loss_fwd_bwd for y, t (B,P) fp32 contiguous:
 * pix (B) receives pix_b, the image's own mean (NOT multiplied by s_b).  A gradient element is the fp64 value
 * tsr_pixel_loss_fwd_bwd rounds for n = B P (dy_scale omega_p rho'(d_p) / (B P)), multiplied last by (double)s_b and
 * rounded once: with s NULL (all ones) or s_b == 1, dy and dt equal the flat launch's bit for bit.  dy (optional) and dt
 * (optional, always overwritten, dt != dy) follow the flat launch's contract.  One workgroup per image, at most max_wgs
 * (TSR_PIXEL_LOSS_PS_MAX_WGS without the _wgs suffix) of them walking the batch at a stride of the grid; the image's sum
 * is fp64 in a fixed order that depends on P alone (thread k of 256 owns elements 4j .. 4j+3 for j = k, k + 256, ...;
 * then the flat launch's workgroup sum); no atomics, no work buffer: neither the cap nor a second launch changes a bit.
 * 16-byte accesses when P % 4 == 0 and y, t and the given dy, dt are 16-byte aligned; otherwise the same elements move one
 * float at a time with the same bits.  1 <= P <= 2^28.  Non-finite pixels stay in their own element and their own pix_b;
 * a NaN s_b makes its image's whole dy and dt NaN.
 * Refusals (status 1 before any device call, nothing written): those of tsr_pixel_loss_fwd_bwd (loss and work aside); B <= 0;
 * P <= 0 or above 2^28; a NULL pix; max_wgs < 1.
 *
 * tsr_ssim_fwd_bwd_ps is tsr_ssim_fwd_bwd with s (B), NULL = all ones: the gradient factor is
 * (double)dy_scale (double)s_b; ssim_b is the image's own value; a skipped image does no window work.  With s NULL or all
 * ones the bits are those of tsr_ssim_fwd_bwd.  Refusals: those of tsr_ssim_fwd_bwd.
 *
 * tsr_weighted_mean: out[0] = fl32((1/B) sum_{s_b != 0} s_b v_b), fp64, in index order; s NULL = the plain mean.  v_b is
 * not read where s_b == 0 (a NaN there never reaches out).  One workgroup.
 * Refusals: tsr_sample_scale a NULL w, s or stats, B <= 0, mode outside {0, 1}; tsr_weighted_mean a NULL v or out, B <= 0. */
#define TSR_PIXEL_LOSS_PS_MAX_WGS 2048
int tsr_sample_scale(const float* w, int B, int mode, float* s, float* stats, void* stream);
int tsr_pixel_loss_ps_fwd_bwd(const float* y, const float* t, int B, long long P, int kind, double param, float fg_weight,
                              float fg_threshold, const float* s, float* pix, float* dy, float dy_scale, int accumulate,
                              float* dt, void* stream);
int tsr_pixel_loss_ps_fwd_bwd_wgs(const float* y, const float* t, int B, long long P, int kind, double param,
                                  float fg_weight, float fg_threshold, const float* s, float* pix, float* dy,
                                  float dy_scale, int accumulate, float* dt, int max_wgs, void* stream);
int tsr_ssim_fwd_bwd_ps(const float* y, const float* t, int B, int H, int W, int win, double sigma, double C1, double C2,
                        const float* s, float* ssim, float* dy, float dy_scale, int accumulate, void* stream);
int tsr_weighted_mean(const float* v, const float* s, int B, float* out, void* stream);

/* Rot90 / flip augmentation on the device (csrc/dihedral.hip; the reference's augmentData, utility/raw_data_process.py:57-95,
 * without storing four copies, plus the mirrored half of the dihedral group): gather sample idx[b] of src and write it
 * transformed, in one pass and one launch.
 *   out[b] = (accumulate ? out[b] : 0) + scale * D_{op[b]}( src[ idx ? idx[b] : b ] )        b < B
 * src (n_src,C,H,W) and out (B,C,H,W) are fp32, contiguous, and must not overlap.  idx (B) is int64 on the device, NULL = the
 * identity; op (B) is int32 on the device, one entry per output sample, NULL = the host argument op_all for every sample.
 * Nothing is read back to the host: the launch can be captured in a HIP graph.  A data path: there is no backward entry.
 * Op code: op = k + 4 f.  f = 1 mirrors along W first; then k counter-clockwise quarter turns are applied exactly as
 * np.rot90(x, k, axes=(-2, -1)), so ops 0..3 are the reference's four.  Output element (i, j) is the source element
 *   (a(u), b(v)), (u, v) = k odd ? (j, i) : (i, j), a(u) = [op & 2] ? H-1-u : u, b(v) = [popcount(op) odd] ? W-1-v : v.
 * Arithmetic: scale == 1 with accumulate = 0 copies the 32-bit patterns (NaN payloads survive); otherwise an element is the
 * one rounding of scale * x (accumulate = 0) or one fmaf(scale, x, out) (accumulate = 1).
 * Channel map (optional): device arrays cmap[8][C] (int32 source channel) and csign[8][C] (float +1 or -1) indexed by op:
 * output plane c is D_op of source plane cmap[op][c], times csign[op][c] before scale.  The sign is applied by flipping the
 * sign bit when csign is negative -- the exact product for +-1, and a NaN keeps its payload; the magnitude is not read.
 * Both NULL: every plane is transformed on its own (the reference).  This carries the "vector" axis mode of
 * functional.dihedral_axis_tables.
 * Safety: a bad device value never becomes an out-of-range access.  op_mask is a host bitmask (bit o = op o may occur).  A
 * sample whose op[b] is outside 0..7 or not in op_mask, whose source index (idx[b], or b itself without idx) is outside
 * [0, n_src), or a plane whose cmap entry is outside [0, C), is written as all-NaN (whatever accumulate says); no other
 * sample is touched.
 * Kernels: planes of at most 64 elements go one thread per output element; planes with H (W + 1) <= 15872 (62 KiB of LDS:
 * up to 125x125, every shape of the project) go one workgroup a plane, larger ones as 64x64 tiles, one workgroup a tile;
 * the op is uniform per workgroup.  Even k reverses rows / columns in registers; odd k (a transpose) stages the plane or
 * tile through LDS (row pitch W + 1, 65) so that the global reads and writes both run along rows; float4 accesses where
 * src and out are 16-byte aligned and W % 4 == 0, one float per lane otherwise.  No atomics: two launches give the same
 * bits.
 * Index arithmetic: offsets inside a sample are 32-bit, so C*H*W <= 2^31 - 1; sample offsets (B*C*H*W, n_src*C*H*W) are
 * 64-bit and cannot overflow under that bound; the grid is capped and walked, so B is not bounded by the launch.
 * Refusals (status 1, before any device call, nothing written): a NULL src or out; B, n_src, C, H or W <= 0; op_mask 0,
 * negative or with bits above 7; an odd-k bit in op_mask while H != W; op NULL with op_all outside 0..7 or not in op_mask;
 * exactly one of cmap / csign; C*H*W > 2^31 - 1; accumulate not 0 or 1; scale NaN. */
int tsr_gather_dihedral(const float* src, int n_src, const long long* idx, const int* op, int op_all, int op_mask,
                        const int* cmap, const float* csign, float* out, int B, int C, int H, int W, float scale,
                        int accumulate, void* stream);
/* The same launch with the caller's grid cap: at most max_wgs workgroups are launched, and a workgroup walks the
 * further work items (elements, planes or tiles) at a stride of the grid -- a caller that shares the device with
 * another stream can leave it CUs, and the walk of every kernel can be run at any size.  The result does not depend
 * on max_wgs, bit for bit.  tsr_gather_dihedral is this with max_wgs = TSR_DIHEDRAL_MAX_WGS.  Refusals: those of
 * tsr_gather_dihedral, and max_wgs <= 0. */
#define TSR_DIHEDRAL_MAX_WGS (1 << 20)
int tsr_gather_dihedral_wgs(const float* src, int n_src, const long long* idx, const int* op, int op_all, int op_mask,
                            const int* cmap, const float* csign, float* out, int B, int C, int H, int W, float scale,
                            int accumulate, int max_wgs, void* stream);

/* Taxel sensor-noise augmentation on the device (csrc/taxel_noise.hip): per-taxel gain drift, heteroscedastic Gaussian
 * read-out noise and dead taxels applied to x (B,C,H,W) fp32 in one launch, driven by a counter-based generator, so the
 * degradation of a sample is a pure function of (seed, offset, sample id, element) -- not of the batch size, the position
 * in the batch, the grid or the code path.
 * Generator: Philox4x32-10.  Multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57; Weyl key increments 0x9E3779B9, 0xBB67AE85;
 * ten rounds  c' = (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),  the key bumped after each round.
 *   key     = (seed_lo, seed_hi)                   the two halves of the 64-bit seed
 *   counter = (block, id, offset, tag)
 * block: the block index inside the sample; id: ids[b] (device int64) or, with ids NULL, id_base + b; offset: a 32-bit
 * stream number (the loader passes its epoch); tag: the effect, 0 = element noise, 1 = gain, 2 = dropout.  One block gives
 * four words r0..r3; lane l of block j serves item 4 j + l of its effect.  An id outside [0, 2^31) makes that sample's
 * output all-NaN and nothing else (the convention of tsr_gather_dihedral for a bad index).
 * Effects, with P = H W, element i = c P + p of a sample, axis = c % axis_cnt (channels are frame-major, axis_cnt axes per
 * frame, the Seqs layout), applied in this order; every fp32 operation rounds once, as written:
 *   gain (tag 1), axis_cnt P items, item axis P + p -- shared by all frames of a sample: drift belongs to the taxel:
 *       u = (r >> 8) 2^-24,  g = fmaf(gain_jitter, 2 u - 1, 1),  v = g x
 *   noise (tag 0), C P items in memory order; words (r0, r1) give items 4 j and 4 j + 1, (r2, r3) items 4 j + 2 and 4 j + 3:
 *       u1 = (2 (ra >> 9) + 1) 2^-24   (exact, never 0: |n| <= 5.77),  u2 = (rb >> 8) 2^-24
 *       R = sqrtf(-2 logf(u1)),  n_a = R cospif(2 u2),  n_b = R sinpif(2 u2)
 *       t = sigma_mul[axis] v,  s = sqrtf(fmaf(t, t, sigma_add[axis]^2)),  y = fmaf(s, n, v)
 *   dropout (tag 2), P items, item p: dead when (r >> 8) < drop_thresh, drop_thresh = round(drop_prob 2^24) in [0, 2^24];
 *       a dead taxel reads drop_value in every channel of the sample (a select: it replaces a NaN too).
 * sigma_add, sigma_mul: HOST arrays of axis_cnt floats, passed to the kernel by value.  A neutral effect is skipped, not
 * computed with zeros: gain_jitter == 0; both sigmas of an axis 0 (per axis); drop_thresh == 0.  With everything neutral
 * out == x bit for bit, NaN payloads and -0 included.  A NaN or Inf in x stays in its own element.
 * out may be x itself (in place) or disjoint from it.  One thread per four consecutive elements; 16-byte loads and stores
 * when P % 4 == 0 and both bases are 16-byte aligned, single dwords otherwise, with the same bits.  No atomics: two
 * launches give the same bits.
 * Refusals (status 1, before any device call, nothing written): a NULL x, out, sigma_add or sigma_mul; B, C, H or W <= 0;
 * axis_cnt outside 1..4 or C % axis_cnt != 0; C*H*W > 2^31 - 1; a negative or non-finite sigma; a non-finite gain_jitter
 * or drop_value; drop_thresh outside [0, 2^24]; x and out overlapping without being equal. */
int tsr_taxel_noise(const float* x, float* out, int B, int C, int H, int W, int axis_cnt, const float* sigma_add,
                    const float* sigma_mul, float gain_jitter, int drop_thresh, float drop_value, const long long* ids,
                    long long id_base, unsigned long long seed, unsigned offset, void* stream);
/* The same launch with the caller's grid cap: at most max_wgs workgroups of 256, each walking the further work items at a
 * stride of the grid.  The result does not depend on max_wgs, bit for bit.  tsr_taxel_noise is this with max_wgs =
 * TSR_TAXEL_NOISE_MAX_WGS.  Refusals: those of tsr_taxel_noise, and max_wgs <= 0. */
#define TSR_TAXEL_NOISE_MAX_WGS (1 << 20)
int tsr_taxel_noise_wgs(const float* x, float* out, int B, int C, int H, int W, int axis_cnt, const float* sigma_add,
                        const float* sigma_mul, float gain_jitter, int drop_thresh, float drop_value, const long long* ids,
                        long long id_base, unsigned long long seed, unsigned offset, int max_wgs, void* stream);
/* The same launch with the generator state read by the kernel from device memory: rng_dev points to four 32-bit words
 * {seed_lo, seed_hi, offset, 0}.  A captured graph draws fresh noise on every replay once the host (or a kernel) rewrites
 * the offset word (the pattern of tsr_ema_multi_dev).  The bits equal tsr_taxel_noise's for the same seed and offset.
 * Refusals: those of tsr_taxel_noise, and a NULL rng_dev. */
int tsr_taxel_noise_dev(const float* x, float* out, int B, int C, int H, int W, int axis_cnt, const float* sigma_add,
                        const float* sigma_mul, float gain_jitter, int drop_thresh, float drop_value, const long long* ids,
                        long long id_base, const unsigned* rng_dev, void* stream);
/* The raw stream: out (B, blocks, 4) receives the four words of blocks 0 .. blocks - 1 of effect `tag` for every sample
 * (id as above; a sample with an id outside [0, 2^31) receives the word 0x7fc00000 throughout).  This is how a caller
 * reproduces the generator.  Refusals: a NULL out, B or blocks <= 0, a negative tag. */
int tsr_taxel_noise_bits(unsigned* out, int B, int blocks, const long long* ids, long long id_base, int tag,
                         unsigned long long seed, unsigned offset, void* stream);

/* Contact readout (csrc/contact_readout.hip): where the contact is, how large, how oriented and how heavy, read out of a
 * pressure image -- and, for a pair (output y, target t), how far the two contacts are apart -- from one launch.  The
 * reference builds its targets from binarised contact masks (utility/raw_data_process.py:105-106 thresholds the depth at
 * 0.5 min + 0.5 max; model/tPSFNet.py:87 calls the result the contact surface); mode 1 at threshold 0.5 is that rule.
 * Per image, all arithmetic in double from the exact fp32 pixels v_p, p = (x, c) in row-major order:
 *   tau   mode 0 ("abs"):   (double)(float)threshold
 *         mode 1 ("range"): mn + threshold (mx - mn), mn / mx the image's own minimum / maximum, evaluated as a separate
 *                           subtraction, product and sum (no fused contraction); y and t each use their own tau
 *   m_p = [(double)v_p > tau]                                       the comparison is strict
 *   u(x) = (x + 0.5) span_r / H - 0.5,  v(c) = (c + 0.5) span_c / W - 0.5     taxel-pitch units, independent of the grid:
 *                                                                    with span = 4 taxel a's centre is at u = a (on the
 *                                                                    100x100 grid pixel 12 + 25 a, the reference's centres)
 * Record (TSR_CONTACT_REC = 16 floats), M0 = sum_p m_p v_p:
 *   [0]  n = sum_p m_p                           [1]  area = n (span_r / H)(span_c / W)
 *   [2]  mass M = gain M0                        [3]  total = gain sum_p v_p              [4]  peak = gain mx
 *   [5], [6]   (u, v) of the first maximum in row-major order
 *   [7], [8]   centroid (cu, cv) = sum_p m_p v_p (u, v) / M0
 *   [9], [10], [11]   muu, mvv, muv = sum_p m_p v_p (u - cu)^2 / M0, ... (v - cv)^2 ..., ... (u - cu)(v - cv) ...
 *   [12] theta = 0.5 atan2(2 muv, muu - mvv) in (-pi/2, pi/2]; exactly 0 when both arguments are 0; a value whose fp32
 *        rounding would be -fl32(pi/2) is stored as +pi/2, the same axis
 *   [13], [14]   sqrt(lambda+), sqrt(lambda-),  lambda+- = (muu + mvv)/2 +- sqrt(((muu - mvv)/2)^2 + muv^2), each clamped
 *                at 0 before the root
 *   [15] tau
 *   With n = 0 or M0 <= 0 the entries 7..14 are NaN; 0..6 and 15 are still valid.
 * The moments are summed about the peak pixel in integer pixel offsets (exact products) and moved to the centroid at the
 * end: a one-pixel contact has moments and axes of exactly 0, never a negative root or a NaN.
 * Pair (TSR_CONTACT_PAIR = 8 floats):
 *   [0]  intersection count sum_p m^y_p m^t_p   [1]  union count n_y + n_t - [0]
 *   [2]  IoU = [0] / [1]; 1 when the union is 0 [3]  Dice = 2 [0] / (n_y + n_t); 1 when both masks are empty
 *   [4]  centroid distance sqrt((cu_y - cu_t)^2 + (cv_y - cv_t)^2); NaN when either contact is empty (has NaN geometry)
 *   [5]  |M_y - M_t| / M_t; NaN when n_t = 0 or M_t <= 0
 *   [6]  distance between the two peak positions
 *   [7]  |theta_y - theta_t| folded into [0, pi/2] (d > pi/2 -> pi - d); NaN when either is NaN
 * y (B,1,H,W) fp32 contiguous.  t optional, the same shape; NULL = one image per sample, rec_t and pair must then be
 * NULL.  rec_y (B,16).  rec_t (B,16), optional when t is given.  pair (B,8), required when t is given.  y and t may be
 * the same buffer.  Every stored value is rounded to fp32 once, at the store; H W <= 2^24 keeps the counts exact.
 * One workgroup of 256 per image (pair), at most TSR_CONTACT_MAX_WGS of them walking the batch at a stride of the grid.
 * Two passes: minimum, maximum, first maximum and a non-finite flag; then counts and moments, re-read from cache.  Thread k
 * owns pixels 4j .. 4j+3 of the flat image for j = k, k + 256, ...; 16-byte loads when W % 4 == 0 and the base is 16-byte
 * aligned, otherwise the same pixels one float at a time through the same arithmetic, with the same bits.  The map and the
 * reduction order (shuffle tree per wave, waves in order) depend on (H, W) alone; no atomics and no host synchronisation:
 * two launches give the same bits, and the launch can be captured in a HIP graph.
 * Non-finite input: images are independent.  An image that holds a NaN or an Inf gets an all-NaN record; when it belongs
 * to a pair, pair is all-NaN too and the clean partner keeps its own valid record.  Every other image keeps the bits of
 * the clean run.  Bad input never causes an out-of-range access.
 * Refusals (status 1, before any device call, nothing written): a NULL y or rec_y; B, H or W <= 0; H W > 2^24; mode outside
 * 0..1; threshold NaN or Inf; mode 1 with threshold outside [0, 1); gain NaN or Inf; span_r or span_c <= 0, NaN or Inf;
 * t NULL with rec_t or pair given; t given without pair; any output overlapping an input or another output. */
#define TSR_CONTACT_REC 16
#define TSR_CONTACT_PAIR 8
#define TSR_CONTACT_MAX_WGS 2048
int tsr_contact_readout(const float* y, const float* t, int B, int H, int W, int mode, double threshold, double gain,
                        double span_r, double span_c, float* rec_y, float* rec_t, float* pair, void* stream);
/* The same launch with the caller's grid cap (tsr_contact_readout is this with max_wgs = TSR_CONTACT_MAX_WGS).  The result
 * does not depend on max_wgs, bit for bit.  Refusals: those above, and max_wgs < 1. */
int tsr_contact_readout_wgs(const float* y, const float* t, int B, int H, int W, int mode, double threshold, double gain,
                            double span_r, double span_c, float* rec_y, float* rec_t, float* pair, int max_wgs,
                            void* stream);

/* ---------------------------------------------------------------------------------------
 * tPSFNet (model/tPSFNet.py): batched, one workgroup per sample (the reference loops over the
 * batch in python, :118-125).  size is fixed at 100x100 depth / 99x99 PSF / 4x4 taxels, as the
 * reference's geometry constants are (:40-55).
 * ------------------------------------------------------------------------------------- */
/* tactilePSF + depth2tactile + degradation_process (:78-100,129-141) from alpha_beta (B,3) =
 * (alpha, beta, gamma): HR (B,1,100,100), LR_deg (B,1,4,4), psf (B,1,99,99).  Separable form.
 * Plateau: the pixels with depth > depth.max() - 1e-3 (never empty in exact arithmetic; evaluated in fp32 like the reference,
 * so a maximum of 2^15 or more, which 1e-3 no longer moves, has none) hold max(HR off the plateau, 0).  Degenerate
 * plateaus follow from that: an image that is all plateau (constant depth, all zeros) gives HR = 0 and LR_deg = 0 exactly,
 * and psf as always; when every pixel off the plateau has a negative HR the plateau holds 0.  Samples are independent: a
 * NaN or Inf in one sample's depth or parameters stays in that sample's outputs.
 * Refusals: a NULL depth, alpha_beta, HR, LR_deg or psf, or B <= 0, returns status 1, launches nothing and leaves every
 * output untouched. */
int tpsf_forward(const float* depth, const float* alpha_beta, float* HR, float* LR_deg, float* psf,
                 int B, void* stream);
/* d loss / d (alpha, beta, gamma) (B,3) given d loss / d LR_deg (B,16); plateau pixels carry no
 * gradient, depth carries none (autograd of :118-125 as used by train/tPSFNet_train.py:180-190).  HR = the forward
 * output of the same (depth, alpha_beta) (tpsf_forward: the reductions over it are not recomputed); work: B*100*100
 * floats of scratch (the per-pixel dL/dHR between the two kernels; exactly 0 on the plateau).  An all-plateau image has
 * exactly zero gradients in all three components.
 * Refusals: a NULL depth, alpha_beta, HR, dLR_deg, d_alpha_beta or work, or B <= 0, returns status 1, launches nothing and
 * leaves d_alpha_beta and work untouched. */
int tpsf_backward(const float* depth, const float* alpha_beta, const float* HR, const float* dLR_deg,
                  float* d_alpha_beta, float* work, int B, void* stream);
/* The full backward of tpsf_forward: upstream gradients of all three outputs -- dLR_deg (B,16), dHR (B,100,100), dpsf
 * (B,99,99), each optional (NULL = none) -- to d_alpha_beta (B,3) and, when d_depth is not NULL, to the depth (B,100,100).
 * Per sample, with D the depth, G[i][j] = g(i-j), g(t) = exp(-Kp t^2 / beta^2) for |t| <= 49 and 0 beyond, Kp = 100/4802, H the
 * Toeplitz matrix of t^2 g(t), P the plateau D > max D - 1e-3 and m_ac(gamma) the normalised pooling mask of taxel (a,c):
 *     W         = [not P] (dHR + 1e-4 sum_ac dLR_deg[a][c] m_ac(gamma))        (what `work` receives; exactly 0 on the plateau)
 *     d/dalpha  = sum W (G D G) + sum dpsf g(u) g(v)                           (the first sum over the stored HR / alpha)
 *     d/dbeta   = alpha (2 Kp / beta^3) (<W, H D G + G D H> + sum dpsf g(u) g(v) (u^2 + v^2))      (u, v from the psf centre)
 *     d/dgamma  = through dLR_deg only: bit for bit tpsf_backward's for the same dLR_deg, an exact 0 without one
 *     d_depth   = alpha G W G             (g is even: the adjoint of the "same" convolution is the same Toeplitz pair)
 * NOT differentiated, as in the reference's autograd: the plateau threshold max D, and the fill value (a detached constant), so
 * plateau pixels of the OUTPUT take no gradient (whatever dHR holds there is ignored) while the INPUT pixels under the plateau
 * do receive their d_depth.  An all-plateau image has d_depth exactly 0 and only the psf terms in d/dalpha, d/dbeta.  With dpsf
 * alone W is 0: d_depth is exactly 0 and `work` is not written.  Samples are independent (NaN / Inf stay in their sample).
 * With dHR, dpsf and d_depth all NULL this is tpsf_backward: the same two launches, d_alpha_beta and work bit for bit.
 * Refusals: a NULL depth, alpha_beta, HR, d_alpha_beta or work, all three upstream pointers NULL, or B <= 0, returns status 1,
 * launches nothing and leaves d_alpha_beta, d_depth and work untouched. */
int tpsf_backward_ex(const float* depth, const float* alpha_beta, const float* HR,
                     const float* dLR_deg /* B*16, NULL = none */, const float* dHR /* B*100*100, NULL = none */,
                     const float* dpsf /* B*99*99, NULL = none */,
                     float* d_alpha_beta, float* d_depth /* B*100*100, NULL = not wanted */,
                     float* work, int B, void* stream);
/* C[i][j] = act(sum_k A(i,k)B(k,j) + bias[j]), A(i,k)=A[i*sa0+k*sa1], B(k,j)=B[k*sb0+j*sb1]; act 0 none,
 * 1 ReLU, 2 Softplus: the nn.Linear layers of MLP_layer (:26-36) and their backward GEMMs.
 * Refusals (the whole family: tsr_sgemm, tsr_sgemm_masked, tsr_sgemm_splitk, tsr_sgemm_splitk_strided, tsr_colsum_splitk): a
 * NULL A, B or C / slab / Y (bias may be NULL; mask_ref may not), M, N or K <= 0, act outside 0..2, nsplit outside 1..65535,
 * or a split_stride below the size of one partial (M*N; N for the column sums) returns status 1, launches nothing and leaves
 * the output untouched. */
int tsr_sgemm(const float* A, long long sa0, long long sa1, const float* B, long long sb0, long long sb1,
              const float* bias, float* C, int M, int N, int K, int act, void* stream);
/* Split-K form for the reductions over the batch (dW = dy^T x, db = 1^T dy of the same layers): slab[s][M][N]
 * receives the partial product of K range s (no bias / activation); add the slabs with tsr_reduce_splits.
 * Range s covers K indices [s*c, min((s+1)*c, K)) with c = ceil(K / nsplit) rounded up to whole 32-deep K steps.  Any nsplit in
 * 1..65535 is valid: a split whose range is empty (nsplit above the number of K steps) still WRITES its partial, as exact
 * zeros, so tsr_reduce_splits over all nsplit partials is always right and a slab needs no clearing.  The same holds for
 * tsr_sgemm_splitk_strided and, with K = M rows, for tsr_colsum_splitk; neither touches the gap between partials. */
int tsr_sgemm_splitk(const float* A, long long sa0, long long sa1, const float* B, long long sb0, long long sb1,
                     float* slab, int M, int N, int K, int nsplit, void* stream);
/* dx GEMM of a layer with the ReLU backward of the layer below fused: C[i][j] = (sum_k A(i,k)B(k,j)) if mask_ref[i][j] > 0
 * else 0 (mask_ref = the stored ReLU output the gradient flows back through, row-major [M][N]). */
int tsr_sgemm_masked(const float* A, long long sa0, long long sa1, const float* B, long long sb0, long long sb1,
                     const float* mask_ref, float* C, int M, int N, int K, void* stream);
/* tsr_sgemm_splitk with a caller-chosen distance between the partial results (split s lands at slab + s*split_stride,
 * split_stride >= M*N): the partials of several GEMMs share one [nsplit][total] buffer that ONE tsr_reduce_splits call
 * adds into a flat gradient buffer. */
int tsr_sgemm_splitk_strided(const float* A, long long sa0, long long sa1, const float* B, long long sb0, long long sb1,
                             float* slab, long long split_stride, int M, int N, int K, int nsplit, void* stream);
/* Column sums of Y[M][N] per row range (db = 1^T dy over the same K ranges as the split-K GEMM with K = M):
 * slab[s*split_stride + j] = sum of rows of range s. */
int tsr_colsum_splitk(const float* Y, float* slab, long long split_stride, int M, int N, int nsplit, void* stream);
/* Which kernel form a launch of the tsr_sgemm family takes (host arithmetic: no launch, no device call; the launches make
 * their choice through the same function).  Returns BM*100 + AF*10 + BF: BM = tile height, 64 or 128 (128 unless
 * ceil(N/128) * ceil(M/128) * nsplit < 384 and M > 64); AF / BF = load path of A / B: 1 = 16-B loads along k (unit stride
 * along k, the other stride and K multiples of 4, pointer 16-B aligned), else 2 = 16-B loads along m / n (unit stride
 * along m / n, the other stride and M / N multiples of 4, pointer 16-B aligned), else 0 = scalar loads.  a_align16 /
 * b_align16: non-zero when the operand's pointer is 16-B aligned.  nsplit = 1 for tsr_sgemm and tsr_sgemm_masked.  Returns 0
 * for what the launches refuse: M, N or K <= 0, nsplit outside 1..65535. */
int tsr_sgemm_form(long long sa0, long long sa1, long long sb0, long long sb1, int a_align16, int b_align16,
                   int M, int N, int K, int nsplit);
/* dy *= act'(.) in place from the stored activation output (1 ReLU, 2 Softplus). */
int tsr_act_bwd(float* dy, const float* y, long long n, int mode, void* stream);

/* Layout plumbing (tests, stage probes): NCHW (B,C,HW) <-> a channel slice of a CB16 buffer. */
int tsr_nchw_to_cb16(const float* src, float* dst, int B, int C, int HW, int dst_ctot, int dst_coff, void* stream);
int tsr_cb16_to_nchw(const float* src, float* dst, int B, int C, int HW, int src_ctot, int src_coff, void* stream);

#ifdef __cplusplus
}
#endif
#endif
