"""Train-mode forward (batch-statistics BatchNorm) and full backward of TactileSR on the HIP
kernels, exposed to autograd as ONE ``torch.autograd.Function`` so that the reference's
step protocol -- ``loss = criterion(model(LR), HR); loss.backward(); optimizer.step()``
(train/tactileSR_train.py:41-51, cpu/trainer.py:346-362) -- works unchanged and ``.grad``
appears on the registered ``nn.Parameter``s.

Forward keeps, per BN layer, only the raw bias-free conv output ``z`` (CB16) plus four
per-channel vectors; ``relu(bn(z))`` is never materialised -- consumers apply it while
staging their input tiles.  Backward = dgrad (the same MFMA conv kernel with flipped /
transposed weights and a ReLU-mask + BN-reduction epilogue) + wgrad (MFMA split-K over the
batch) + a small elementwise BN-backward pass per BN layer.
"""
from __future__ import annotations

import ctypes
from ctypes import c_int, c_void_p, c_float, c_double, c_longlong, POINTER, byref
from typing import NamedTuple

import torch

from .. import _lib
from .._lib import call, ptr, stream
from .tactileSR_model import (NS_F32, NS_F16X3, NS_B16, NS_B16K, NS_B16K_PAIR, _SlotPool, _timed, _twin_args, _pack_form,
                              _pack_pair_b16k, to_cb16, from_cb16)

_I, _F, _D, _L = c_int, c_float, c_double, c_longlong


# tsr_head_bwd keeps the zero-padded H x W head gradient in 64 KB of LDS: outputs up to 126 x 126 (4 x 4 taxels: sf <= 31)
HEAD_BWD_LDS_BYTES = 64 * 1024


def check_trainable_size(H, W):
    """Raise before the train step launches anything when its H x W output is beyond the library's train kernels."""
    if (H + 2) * (W + 2) * 4 > HEAD_BWD_LDS_BYTES:
        raise _lib.TactileSRHipError(
            f"train step at {H}x{W} output: tsr_head_bwd needs (H+2)*(W+2)*4 <= {HEAD_BWD_LDS_BYTES} bytes of LDS "
            f"(at most 126x126, scale_factor <= 31 on 4x4 taxels)")


# ---------------------------------------------------------------------------------------------------------------------
# Backward plan (host only: no device, no library).  One record per launch of TrainEngine.backward / BlockEngine.backward in
# the order the engines issue them.  Labels name gradient tensors; a "saved:" label is a tensor the forward kept (or the
# incoming dout) and has no producer.  The BatchNorm sums a dgrad(bn=True) epilogue leaves in the statistics slab are an
# output of that dgrad (label "<tensor>.sums"), consumed by the bn_bwd_finalize behind it; the coefficients a finalize
# writes ("<bn>.coef") are consumed by its bn_bwd_apply, which turns the masked gradient g into dz in place.
# A BatchNorm layer in eval mode inside the training module (`bn_eval`: its path; running statistics, dz = scale * g) has
# a bn_bwd_apply that needs no coefficients and a bn_bwd_finalize that only serves dgamma / dbeta: when neither is wanted
# the finalize goes and the dgrad in front of it leaves no sums.
# ---------------------------------------------------------------------------------------------------------------------
class Record(NamedTuple):
    kind: str           # head_bwd | head_dgrad | wgrad | dgrad | bn_bwd_finalize | bn_bwd_apply | stem_wgrad | stem_dgrad
    layer: str          # module path of the conv / BatchNorm (+ "[a:b]" for a dgrad over an input-channel slice)
    consumes: tuple     # gradient-tensor labels read
    produces: tuple     # gradient-tensor labels written
    params: tuple       # parameter-gradient names the launch (and its tsr_reduce_splits) produces

    @property
    def key(self):
        return self.kind, self.layer


def _res_records(p, dpre):
    """Launches of `_res_bwd` for the ResBlock with parameter prefix `p` ("" or "path."); `dpre` labels its incoming gradient."""
    d1, dx = p + "d1", p + "dx"
    return [
        Record("wgrad", p + "conv2", (dpre,), (), (p + "conv2.weight", p + "conv2.bias")),
        Record("dgrad", p + "conv2", (dpre,), (d1,), ()),
        Record("wgrad", p + "conv1", (d1,), (), (p + "conv1.weight", p + "conv1.bias")),
        Record("dgrad", p + "conv1", (d1, dpre), (dx,), ()),
    ]


def bn_members(layer):
    """Module paths of the BatchNorm layers behind a record's `layer`: itself, or for layers that share a launch
    ("<block>.conv_3_1.1|conv_5_1.1", the stage-1 pair of an MSRB) each of them."""
    head, _, tail = layer.partition("|")
    return (head, head[:len(head) - len(tail)] + tail) if tail else (head,)


def bn_held(layer, bn_eval):
    """Whether the BatchNorm record `layer` runs the eval-mode backward: every layer behind it is in `bn_eval` (a mixed
    stage-1 pair keeps the batch-statistics launches; the engine zeroes the statistics terms of its held half)."""
    return all(n in bn_eval for n in bn_members(layer))


def _bn_records(bn, g, dz, params, bn_eval):
    """The two BatchNorm-backward records behind the dgrad that left the masked gradient `g` and its sums."""
    if bn_held(bn, bn_eval):
        return [Record("bn_bwd_finalize", bn, (g + ".sums",), (), params), Record("bn_bwd_apply", bn, (g,), (dz,), ())]
    return [Record("bn_bwd_finalize", bn, (g + ".sums",), (bn + ".coef",), params),
            Record("bn_bwd_apply", bn, (g, bn + ".coef"), (dz,), ())]


def _msrb_records(p, dpre, virtual, bn_eval=frozenset()):
    """Launches of `_msrb_bwd` for the MSRB with parameter prefix `p`; `virtual`: the block input is relu(bn(z)) of the layer
    below, so the last dgrad's epilogue also leaves that BatchNorm's backward sums."""
    recs = [Record("wgrad", p + "confusion", (dpre,), (), (p + "confusion.weight", p + "confusion.bias"))]
    for o, nm in ((0, "conv_3_2"), (128, "conv_5_2")):
        sl = f"[{o}:{o + 128}]"
        g, dz, bn = p + "g2" + sl, p + "dz2" + sl, p + nm + ".1"
        recs += [Record("dgrad", p + "confusion" + sl, (dpre,), (g, g + ".sums"), ())]
        recs += _bn_records(bn, g, dz, (bn + ".weight", bn + ".bias"), bn_eval)
    dz32, dz52 = p + "dz2[0:128]", p + "dz2[128:256]"
    bn1 = p + "conv_3_1.1|conv_5_1.1"
    recs += [
        Record("wgrad", p + "conv_3_2.0", (dz32,), (), (p + "conv_3_2.0.weight", p + "conv_3_2.0.bias")),
        Record("wgrad", p + "conv_5_2.0", (dz52,), (), (p + "conv_5_2.0.weight", p + "conv_5_2.0.bias")),
        Record("dgrad", p + "conv_3_2.0", (dz32,), (p + "g1.3",), ()),
        Record("dgrad", p + "conv_5_2.0", (dz52, p + "g1.3"), (p + "g1", p + "g1.sums"), ())]
    recs += _bn_records(bn1, p + "g1", p + "dz1", (p + "conv_3_1.1.weight", p + "conv_3_1.1.bias", p + "conv_5_1.1.weight",
                                                   p + "conv_5_1.1.bias"), bn_eval)
    recs += [
        Record("wgrad", p + "conv_3_1.0", (p + "dz1",), (), (p + "conv_3_1.0.weight", p + "conv_3_1.0.bias")),
        Record("wgrad", p + "conv_5_1.0", (p + "dz1",), (), (p + "conv_5_1.0.weight", p + "conv_5_1.0.bias")),
        Record("dgrad", p + "conv_3_1.0", (p + "dz1", dpre), (p + "dx.3",), ()),
        Record("dgrad", p + "conv_5_1.0", (p + "dz1", p + "dx.3"), (p + "dx",) + ((p + "dx.sums",) if virtual else ()), ()),
    ]
    return recs


def _prune(recs, want, want_out):
    """The records that something wanting a gradient depends on: one of its parameter gradients is in `want`, or one of its
    outputs is in `want_out` or is consumed by a kept record (one sweep from the back: consumers follow producers).  A kept
    head_bwd whose weight gradient nobody wants becomes head_dgrad (tsr_head_dgrad: the same dz_h0, no weight partials); a
    kept dgrad whose BatchNorm sums nobody reads (an eval-mode BatchNorm with gamma and beta frozen) loses that output."""
    need, keep = set(want_out), []
    for r in reversed(recs):
        if any(n in want for n in r.params) or any(t in need for t in r.produces):
            need.update(r.consumes)
            if r.kind == "head_bwd" and not any(n in want for n in r.params):
                r = Record("head_dgrad", r.layer, r.consumes, r.produces, ())
            if r.kind == "dgrad" and any(t.endswith(".sums") and t not in need for t in r.produces):
                r = r._replace(produces=tuple(t for t in r.produces if not t.endswith(".sums") or t in need))
            keep.append(r)
    keep.reverse()
    return keep


def backward_plan(seqsCnt, n_msrb, n_res, want, want_dx=False, bn_eval=frozenset()):
    """Launch list of `TrainEngine.backward` for a TactileSR of `seqsCnt` frames, `n_msrb` MSRBs and `n_res` ResBlocks when
    the parameter gradients named in `want` (and, with `want_dx`, the taxel gradient "LR.grad") are asked for.  `want` = every
    parameter name gives the unfiltered list: the all-trainable step.  `bn_eval`: module paths of the BatchNorm layers that
    are in eval mode (running statistics held)."""
    bn_eval = frozenset(bn_eval)
    recs = [Record("head_bwd", "output_layer.2", ("saved:dout",), ("dz_h0",), ("output_layer.2.weight",)),
            Record("wgrad", "output_layer.0", ("dz_h0",), (), ("output_layer.0.weight",)),
            Record("dgrad", "output_layer.0", ("dz_h0",), ("g_hcat[0:64]", "g_hcat[64:128]"), ())]
    dpre = "g_hcat[0:64]"
    for i in reversed(range(n_res)):
        p = f"forceFeatureExtra_layer.{i}."
        recs += _res_records(p, dpre)
        dpre = p + "dx"
    recs += [Record("stem_wgrad", "input_layer_force.1", (dpre,), (), ("input_layer_force.1.weight",)),
             Record("stem_dgrad", "input_layer_force.1", (dpre,), ("LR.grad",), ())]
    dpre = "g_hcat[64:128]"
    for i in reversed(range(n_msrb)):
        p = f"patternFeatureExtra_layer.{i}."
        recs += _msrb_records(p, dpre, virtual=(i == 0), bn_eval=bn_eval)
        dpre = p + "dx"
    bn = "inputContact_layer.1"
    recs += _bn_records(bn, dpre, "dzf", (bn + ".weight", bn + ".bias"), bn_eval)
    recs += [Record("wgrad", "inputContact_layer.0", ("dzf",), (), ("inputContact_layer.0.weight",))]
    for t in range(seqsCnt):
        p = f"inputLayer_pattern_list.{t}."
        sl = f"[{64 * t}:{64 * t + 64}]"
        gT, dzT = "gT" + sl, "dzT" + sl
        recs += [Record("dgrad", "inputContact_layer.0" + sl, ("dzf",), (gT, gT + ".sums"), ())]
        recs += _bn_records(p + "5", gT, dzT, (p + "5.weight", p + "5.bias"), bn_eval)
        recs += [Record("wgrad", p + "4", (dzT,), (), (p + "4.weight",)),
                 Record("dgrad", p + "4", (dzT,), (p + "g1", p + "g1.sums"), ())]
        recs += _bn_records(p + "2", p + "g1", p + "dz1", (p + "2.weight", p + "2.bias"), bn_eval)
        recs += [Record("stem_wgrad", p + "1", (p + "dz1",), (), (p + "1.weight",)),
                 Record("stem_dgrad", p + "1", (p + "dz1",), ("LR.grad",), ())]
    return _prune(recs, frozenset(want), ("LR.grad",) if want_dx else ())


def block_backward_plan(kind, want, want_dx=True, bn_eval=frozenset()):
    """`backward_plan` for a standalone ``MSRB`` (`kind` "msrb") / ``ResBlock`` ("res"): parameter names carry no prefix, the
    incoming gradient is "saved:dpre" and "dx" is the gradient of the block input."""
    recs = _msrb_records("", "saved:dpre", False, frozenset(bn_eval)) if kind == "msrb" else _res_records("", "saved:dpre")
    return _prune(recs, frozenset(want), ("dx",) if want_dx else ())


class ConvDesc(ctypes.Structure):
    """Mirror of ``tsr_conv_desc`` (include/tactilesr_hip.h)."""
    _fields_ = [
        ("in_", c_void_p), ("in_ctot", c_int), ("in_coff", c_int), ("cin", c_int),
        ("w_packed", c_void_p), ("cout", c_int), ("ks", c_int),
        ("scale", c_void_p), ("shift", c_void_p),
        ("res", c_void_p), ("res_ctot", c_int), ("res_coff", c_int),
        ("out", c_void_p), ("out_ctot", c_int), ("out_coff", c_int), ("relu", c_int),
        ("B", c_int), ("H", c_int), ("W", c_int),
        ("in_scale", c_void_p), ("in_shift", c_void_p),
        ("res_scale", c_void_p), ("res_shift", c_void_p),
        ("epi_mode", c_int),
        ("mask", c_void_p), ("mask_ctot", c_int), ("mask_coff", c_int),
        ("mask_scale", c_void_p), ("mask_shift", c_void_p),
        ("bn_a", c_void_p), ("bn_b", c_void_p),
        ("slab", c_void_p), ("slab_cnt", c_void_p),
        ("nsplit", c_int),
        ("in_amax", c_void_p), ("w_inv_scale", c_float), ("out_amax", c_void_p), ("w_amax", c_void_p),
    ]


def _p(t):
    return None if t is None else ptr(t).value


class Act:
    """A CB16 activation slice, optionally 'virtual': value = relu(buf*scale+shift)."""
    __slots__ = ("buf", "ctot", "coff", "c", "scale", "shift", "xa", "xb", "amax", "mat")

    def __init__(self, buf, ctot, coff, c, scale=None, shift=None, xa=None, xb=None, amax=None):
        self.buf, self.ctot, self.coff, self.c = buf, ctot, coff, c
        self.scale, self.shift, self.xa, self.xb = scale, shift, xa, xb
        self.amax = amax     # fp16x3 only: 1-element device tensor holding max|buf| (of the raw stored values)
        self.mat = None      # bf16 storage: the materialised relu(buf*scale+shift) once a kernel needed it plain


def conv_ex(*, B, H, W, src: Act, w, cout, ks, out, out_ctot, out_coff, scale=None, shift=None, relu=0,
            res: Act = None, epi_mode=0, mask: Act = None, bn=False, slab=None, slab_cnt=None, nsplit=0,
            w_inv_scale=1.0, out_amax=None, w_amax=None):
    d = ConvDesc()
    d.nsplit = nsplit
    d.in_amax, d.w_inv_scale, d.out_amax, d.w_amax = _p(src.amax), w_inv_scale, _p(out_amax), _p(w_amax)
    d.in_, d.in_ctot, d.in_coff, d.cin = _p(src.buf), src.ctot, src.coff, src.c
    d.w_packed, d.cout, d.ks = _p(w), cout, ks
    d.scale, d.shift = _p(scale), _p(shift)
    if res is not None:
        d.res, d.res_ctot, d.res_coff = _p(res.buf), res.ctot, res.coff
        d.res_scale, d.res_shift = _p(res.scale), _p(res.shift)
    d.out, d.out_ctot, d.out_coff, d.relu = _p(out), out_ctot, out_coff, int(relu)
    d.B, d.H, d.W = B, H, W
    d.in_scale, d.in_shift = _p(src.scale), _p(src.shift)
    d.epi_mode = epi_mode
    if mask is not None:
        d.mask, d.mask_ctot, d.mask_coff = _p(mask.buf), mask.ctot, mask.coff
        d.mask_scale, d.mask_shift = _p(mask.scale), _p(mask.shift)
        if bn:
            d.bn_a, d.bn_b = _p(mask.xa), _p(mask.xb)
    d.slab, d.slab_cnt = _p(slab), _p(slab_cnt)
    st = _lib.load().tsr_conv2d_ex(byref(d), stream())
    if st != 0:
        raise _lib.TactileSRHipError(f"tsr_conv2d_ex failed: status {st}")


def _pack_dev(w, ints, nsplit, w_amax):
    """Pack `w` for a train launch of arithmetic `nsplit` (fp16 planes: scaled from the device scalar `w_amax`); `ints`:
    (cout, cin, ks) for the forward conv, (cout, cin, ks, ci0, nprime) for d(input)[ci0:ci0+nprime]."""
    dgrad = len(ints) == 5
    out, cin = (ints[4], ints[0]) if dgrad else ints[:2]
    name, n, dtype, tail = _pack_form(nsplit, out, cin, ints[2], dgrad=dgrad, dev_amax=True)
    wp = torch.empty(n, dtype=dtype, device=w.device)
    call(name, ptr(w), ptr(wp), *map(_I, ints), *((ptr(w_amax),) if nsplit == NS_F16X3 else tail), stream())
    return wp


def _pack(w, cout, cin, ks, nsplit=0, w_amax=None):
    return _pack_dev(w, (cout, cin, ks), nsplit, w_amax)


def _pack_dgrad(w, cout, cin, ks, ci0, nprime, nsplit=0, w_amax=None):
    return _pack_dev(w, (cout, cin, ks, ci0, nprime), nsplit, w_amax)


TRAIN_IMPLS = {"f32": NS_F32, "bf16x6": 3, "fp16x3": NS_F16X3, "bf16": NS_B16, "bf16op": 1}


class _Ctx:
    """Everything backward needs (device buffers stay alive through this object)."""


class TrainEngine:
    """Runs one train-mode forward / backward of a ``TactileSR`` module."""

    def __init__(self, model, impl: str = "fp16x3"):
        self.m = model
        self.debug = None        # tools may set a dict: backward then stores clones of dz tensors in it
        self.keep_ctx = False    # tests: keep the last forward's context alive in `last_ctx` (activation_masks)
        self.last_ctx = None
        # gradient arena (tactilesr_amd.ddp): one flat buffer in backward-production order; weight gradients are
        # reduced straight into it, so p.grad addresses are stable across steps (the fused Adam's table is built
        # once) and a GradSync can put finished buckets on the wire from inside backward
        self.arena = None
        self.grad_sync = None
        self.n_buckets = 8
        self.profile = None      # bench.py: dict -> HIP-event brackets per launch family, on the launch stream
        # conv arithmetic of the train path (chosen EXPLICITLY: `TactileSR(train_impl=...)` / `model.train_impl = ...`;
        # no environment variable changes it): "f32" = fp32 MFMA, "bf16x6" = split-bf16 (six products, fp32-equivalent),
        # "fp16x3" = two scaled fp16 planes (three products; operand scales from device-side max|.| scalars),
        # "bf16" = BASELINE's "bf16" configurations -- every stored activation / gradient tensor is bf16 CB16 (saved
        #      pre-activations z, dz, dgrad outputs), plain bf16 MFMA operands, fp32 accumulation, fp32 master weights,
        #      BatchNorm statistics, weight gradients and Adam (the reference's reduced-precision switch is the unused
        #      fp16 autocast of cpu/trainer.py:96,203,346-362); "bf16op" = bf16 operands on fp32 tensors (A/B only)
        if impl not in TRAIN_IMPLS:
            raise _lib.TactileSRHipError(f"train_impl {impl!r}: expected one of {sorted(TRAIN_IMPLS)}")
        self.impl = impl
        self.nsplit = TRAIN_IMPLS[impl]
        self.f16 = self.nsplit == NS_F16X3
        self.io16 = self.nsplit == NS_B16
        self.act_dtype = torch.bfloat16 if self.io16 else torch.float32

    def _mfma_convs(self):
        m = self.m
        cv = [m.inputContact_layer[0], m.output_layer[0]]
        cv += [seq[4] for seq in m.inputLayer_pattern_list]
        for blk in m.patternFeatureExtra_layer:
            cv += [blk.conv_3_1[0], blk.conv_5_1[0], blk.conv_3_2[0], blk.conv_5_2[0], blk.confusion]
        for rb in m.forceFeatureExtra_layer:
            cv += [rb.conv1, rb.conv2]
        return cv

    def _weight_scales(self, c):
        """fp16x3: max|w| per conv weight as DEVICE scalars (one batched launch, no host round trip); the pack kernels
        and the convolutions derive the same power-of-two scale (max|w|*wscale in [2^13, 2^14)) from them."""
        c.wamax = {}
        if not self.f16:
            return
        cv = self._mfma_convs()
        mx = torch.stack(torch._foreach_norm([k.weight.detach() for k in cv], float("inf")))
        for i, k in enumerate(cv):
            c.wamax[id(k)] = mx[i:i + 1]

    def _amax_slots(self):
        return 64 + 8 * (len(self.m.patternFeatureExtra_layer) + len(self.m.forceFeatureExtra_layer) + self.m.seqsCnt)

    def _amax_pool(self, dev):
        return _SlotPool(self._amax_slots(), dev, self.f16)

    # ------------------------------------------------------------------ helpers
    def _bn_finalize(self, c: _Ctx, conv_bias, bn, slab, cnt, entries, C):
        dev = slab.device
        vec = torch.empty(4, C, dtype=torch.float32, device=dev)
        call("tsr_bn_stats_finalize", ptr(slab), ptr(cnt), _I(entries), _I(C),
             ptr(conv_bias.detach() if conv_bias is not None else None), ptr(bn.weight.detach()),
             ptr(bn.bias.detach()), ptr(bn.running_mean), ptr(bn.running_var), _F(bn.momentum), _F(bn.eps),
             ptr(vec[0]), ptr(vec[1]), ptr(vec[2]), ptr(vec[3]), ptr(c.work), stream())
        c.nbt.append(bn.num_batches_tracked)      # (+1 for all of them in one launch at the end of forward)
        return vec   # rows: scale, shift, xhat_a, xhat_b

    @staticmethod
    def _bn_eval_vectors(bias, gamma, beta, rm, rv, eps, C):
        """The 4xC BN vectors of a BatchNorm layer in eval mode (``bn.eval()`` inside the training module): from the running
        statistics, which stay as they are -- no statistics pass, no num_batches_tracked bump."""
        vec = torch.empty(4, C, dtype=torch.float32, device=gamma.device)
        call("tsr_bn_eval_vectors", ptr(bias), ptr(gamma), ptr(beta), ptr(rm), ptr(rv), _F(eps), _I(C),
             ptr(vec[0]), ptr(vec[1]), ptr(vec[2]), ptr(vec[3]), stream())
        return vec

    def _bn_held_vec(self, conv_bias, bn, C):
        return self._bn_eval_vectors(conv_bias.detach() if conv_bias is not None else None, bn.weight.detach(),
                                     bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps, C)

    @staticmethod
    def _bump_nbt(c):
        """num_batches_tracked += 1 of every BatchNorm layer the forward ran, as ONE launch (27 one-element launches before)."""
        if c.nbt:
            torch._foreach_add_(c.nbt, 1)
            c.nbt = []

    def _twin(self, name, *args, amax=()):
        """A glue launch in the engine's storage type: `name + "_b16"` under bf16 storage, else `name` with its `amax` pointer."""
        call(*_twin_args(self.io16, name, args, amax), stream())

    def _stem(self, x, ctot_in, coff, A, hin, win, sf, w, dst, relu, B, am):
        """bilinear x sf + conv 3 -> 64 (raw or ReLU'd) into a 64-channel CB16 buffer of the engine's storage type."""
        self._twin("tsr_stem_fwd", ptr(x), _I(ctot_in), _I(coff), _I(A), _I(hin), _I(win), _I(sf), ptr(w), ptr(None),
                   ptr(None), ptr(dst), _I(64), _I(0), _I(relu), _I(B), amax=(am,))

    def _entries(self, c, cout, ks, nsplit):
        """Statistics-slab entries the conv launch (cout, ks) of the form `nsplit` writes."""
        return _lib.load().tsr_conv2d_slab_entries_ex(c.B, c.H, c.W, cout, ks, nsplit)

    def _plain(self, c, a: Act) -> Act:
        """bf16 storage: `a` as a tensor the LDS-DMA kernels (conv_b16k / wgrad_b16k: operands go from HBM to LDS as stored)
        can read -- a virtual activation relu(buf*scale+shift) is materialised ONCE (tsr_bn_relu_b16) and kept on the Act:
        the forward convs of an MSRB's second stage and, in backward, their weight gradients all read the same tensor."""
        if a.scale is None:
            return a
        if a.mat is None:
            a.mat = torch.empty(c.B * a.c * c.HW, dtype=torch.bfloat16, device=a.buf.device)
            call("tsr_bn_relu_b16", ptr(a.buf), _I(a.ctot), _I(a.coff), _I(a.c), ptr(a.scale), ptr(a.shift), ptr(a.mat),
                 _I(c.B), _I(c.HW), stream())
        return Act(a.mat, a.c, 0, a.c)

    def _b16k(self, cout, cin, ks):
        """bf16 storage: this forward conv shape runs csrc/conv_b16k.hip (tsr_conv2d_ex, NS_B16K)."""
        return self.io16 and ks > 1 and bool(_lib.load().tsr_conv2d_ex_dgrad_b16k(cout, cin, ks))

    def _form(self, c, conv, src: Act, dgrad=None):
        """What a training conv launches: (source, packed weight, device scalar max|w| or None, `nsplit` code of the launch).
        `dgrad` None: the forward conv of `conv` on `src`.  Under bf16 storage, the 3x3 / 5x5 shapes csrc/conv_b16k.hip has
        run there (NS_B16K) on a plain source -- a virtual one is materialised -- and the 1x1 shapes csrc/conv1x1_b16k.hip
        has run there on the source as it is: that kernel transforms a virtual input in LDS behind the DMA.
        `dgrad` = (ci0, nprime, plain): d(input)[ci0:ci0+nprime] given dz = `src`; under bf16 storage conv_b16k runs it
        (same tensors, its own pack) when the launch's tensors are `plain` and the kernel has the flipped shape.
        Everything else runs the engine's arithmetic."""
        w = conv.weight.detach().contiguous()
        cout, cin, ks = w.shape[0], w.shape[1], w.shape[2]
        wa = c.wamax.get(id(conv))
        ints = (cout, cin, ks)
        if dgrad is not None:
            ci0, nprime, plain = dgrad
            ints += (ci0, nprime)
            b16k = self.io16 and plain and _lib.load().tsr_conv2d_ex_dgrad_b16k(nprime, cout, ks)
        elif ks > 1:
            b16k = self._b16k(cout, cin, ks)
            if b16k:
                src = self._plain(c, src)
        else:
            b16k = self.io16 and _lib.load().tsr_conv2d_ex_fwd1x1_b16k(cout, cin)
        ns = NS_B16K if b16k else self.nsplit
        return src, _pack_dev(w, ints, ns, wa), wa, ns

    def _pair_bn(self, c: _Ctx, X: Act, blk, cat1):
        """bf16 storage: conv_3_1 || conv_5_1 of an MSRB (reference model/tactileSR_model.py:198-200) as ONE 5x5 launch with
        128 output channels on conv_b16k (tsr_conv2d_ex, NS_B16K_PAIR: the 3x3 weight sits in the inner taps of its half) and
        ONE statistics pass over the 128 channels; returns the 4x128 BN vectors [conv_3_1 | conv_5_1]."""
        c3, b3, c5, b5 = blk.conv_3_1[0], blk.conv_3_1[1], blk.conv_5_1[0], blk.conv_5_1[1]
        if b3.momentum != b5.momentum or b3.eps != b5.eps or (c3.bias is None) != (c5.bias is None):
            raise _lib.TactileSRHipError("stage-1 pair: the two conv + BatchNorm layers differ in momentum / eps / bias")
        cin = c3.weight.shape[1]
        wp = _pack_pair_b16k(c3.weight.detach(), c5.weight.detach())
        with _timed(self.profile, ("fwd", 5, 128, cin)):
            # (the pair form only knows epi_mode 1: with both layers in eval mode its statistics slab is simply not read)
            conv_ex(B=c.B, H=c.H, W=c.W, src=self._plain(c, X), w=wp, cout=128, ks=5, out=cat1, out_ctot=128, out_coff=0,
                    epi_mode=1, slab=c.slab, slab_cnt=c.slab_cnt, nsplit=NS_B16K_PAIR)
        cat = lambda a, b: torch.cat([a.detach(), b.detach()])
        vec = torch.empty(4, 128, dtype=torch.float32, device=wp.device)
        rm, rv = cat(b3.running_mean, b5.running_mean), cat(b3.running_var, b5.running_var)
        bias = cat(c3.bias, c5.bias) if c3.bias is not None else None
        gamma, beta = cat(b3.weight, b5.weight), cat(b3.bias, b5.bias)     # (named: a temporary's block would be reused)
        held = (not b3.training, not b5.training)
        if any(held):
            ev = self._bn_eval_vectors(bias, gamma, beta, rm, rv, b3.eps, 128)      # (before the finalize below moves rm / rv)
            if all(held):
                return ev
        call("tsr_bn_stats_finalize", ptr(c.slab), ptr(c.slab_cnt), _I(self._entries(c, 128, 5, NS_B16K_PAIR)), _I(128),
             ptr(bias), ptr(gamma), ptr(beta), ptr(rm), ptr(rv), _F(b3.momentum), _F(b3.eps),
             ptr(vec[0]), ptr(vec[1]), ptr(vec[2]), ptr(vec[3]), ptr(c.work), stream())
        for h, bnm, sl in ((held[0], b3, slice(0, 64)), (held[1], b5, slice(64, 128))):
            if h:          # a mixed pair: this half keeps its statistics and takes the running-statistics vectors
                vec[:, sl] = ev[:, sl]
                continue
            bnm.running_mean.copy_(rm[sl])
            bnm.running_var.copy_(rv[sl])
            c.nbt.append(bnm.num_batches_tracked)
        return vec

    def _conv_bn(self, c: _Ctx, src: Act, conv, bn, out, out_ctot, out_coff, out_amax=None):
        """conv (bias-free raw output) + batch statistics; returns the 4xC BN vectors."""
        w = conv.weight
        cout, cin, ks = w.shape[0], w.shape[1], w.shape[2]
        src, wp, wis, ns = self._form(c, conv, src)
        if not bn.training:      # eval-mode BatchNorm: the raw output alone (epi_mode 0, no scale / shift / ReLU), no statistics
            with _timed(self.profile, ("fwd", ks, cout, cin)):
                conv_ex(B=c.B, H=c.H, W=c.W, src=src, w=wp, cout=cout, ks=ks, out=out, out_ctot=out_ctot,
                        out_coff=out_coff, nsplit=ns, w_amax=wis, out_amax=out_amax)
            return self._bn_held_vec(conv.bias, bn, cout)
        with _timed(self.profile, ("fwd", ks, cout, cin)):
            conv_ex(B=c.B, H=c.H, W=c.W, src=src, w=wp, cout=cout, ks=ks, out=out, out_ctot=out_ctot,
                    out_coff=out_coff, epi_mode=1, slab=c.slab, slab_cnt=c.slab_cnt, nsplit=ns,
                    w_amax=wis, out_amax=out_amax)
        return self._bn_finalize(c, conv.bias, bn, c.slab, c.slab_cnt, self._entries(c, cout, ks, ns), cout)

    # ------------------------------------------------------------------ forward
    def _new_ctx(self, B, H, W, dev):
        """Per-forward context: geometry + the statistics slabs / workspace every BatchNorm layer reuses."""
        c = _Ctx()
        HW = H * W
        c.B, c.H, c.W, c.HW = B, H, W, HW
        c.nbt = []          # BatchNorm num_batches_tracked counters this forward updates (bumped together: _bump_nbt)
        # BatchNorm layers in eval mode (nn.BatchNorm2d.eval() inside the training module): running statistics, left alone
        root = self.m if self.m is not None else self.block
        c.bn_eval = frozenset(n for n, mod in root.named_modules()
                              if isinstance(mod, torch.nn.BatchNorm2d) and not mod.training)
        lib = _lib.load()
        c.entries = lib.tsr_conv2d_slab_entries(B, H, W)
        c.st_entries = st_entries = lib.tsr_cb16_stats_entries(B, HW)
        # statistics slabs are indexed by (workgroup, image slot): the entry count depends on how many images the
        # kernel variant of (C_out, k, arithmetic) puts in a workgroup -- ask the library for every shape in use
        e64 = max(lib.tsr_conv2d_slab_entries_ex(B, H, W, 64, k, self.nsplit) for k in (1, 3, 5))
        e128 = max(c.entries, max(lib.tsr_conv2d_slab_entries_ex(B, H, W, 128, k, self.nsplit) for k in (1, 3, 5)))
        if self.io16:
            e128 = max(e128, lib.tsr_conv2d_slab_entries_ex(B, H, W, 128, 1, NS_B16K))
        c.slab = torch.empty(max(e128 * 128 * 2, e64 * 64 * 2, st_entries * 64 * 2), dtype=torch.float32, device=dev)
        c.slab_cnt = torch.empty(max(e128, e64, st_entries), dtype=torch.float32, device=dev)
        c.work = torch.empty(512 * 128 * 3, dtype=torch.float64, device=dev)
        return c

    # ------------------------------------------------------------------ blocks (shared with the standalone modules)
    def _msrb_fwd(self, c, blk, X: Act, out, octot, ocoff, am_o, new_amax, buf):
        """One MSRB in train mode (reference model/tactileSR_model.py:196-206): X -> `out[ocoff:ocoff+64]`."""
        dev = X.buf.device
        s = _Ctx()
        s.X = X
        s.cat1, s.cat2 = buf(128), buf(256)
        s.bn_c1 = torch.empty(4, 128, dtype=torch.float32, device=dev)
        s.bn_c2 = torch.empty(4, 256, dtype=torch.float32, device=dev)
        am_c1, am_c2 = new_amax(), new_amax()
        if self._b16k(128, X.c, 5) and blk.conv_3_1[0].weight.shape[0] == 64:
            s.bn_c1[:] = self._pair_bn(c, X, blk, s.cat1)
        else:
            s.bn_c1[:, 0:64] = self._conv_bn(c, X, blk.conv_3_1[0], blk.conv_3_1[1], s.cat1, 128, 0, am_c1)
            s.bn_c1[:, 64:128] = self._conv_bn(c, X, blk.conv_5_1[0], blk.conv_5_1[1], s.cat1, 128, 64, am_c1)
        A1 = Act(s.cat1, 128, 0, 128, s.bn_c1[0], s.bn_c1[1], s.bn_c1[2], s.bn_c1[3], amax=am_c1)
        s.bn_c2[:, 0:128] = self._conv_bn(c, A1, blk.conv_3_2[0], blk.conv_3_2[1], s.cat2, 256, 0, am_c2)
        s.bn_c2[:, 128:256] = self._conv_bn(c, A1, blk.conv_5_2[0], blk.conv_5_2[1], s.cat2, 256, 128, am_c2)
        A2 = Act(s.cat2, 256, 0, 256, s.bn_c2[0], s.bn_c2[1], s.bn_c2[2], s.bn_c2[3], amax=am_c2)
        s.A1, s.A2 = A1, A2
        src, wp, wis, nsc = self._form(c, blk.confusion, A2)
        with _timed(self.profile, ("fwd", 1, 64, 256)):
            conv_ex(B=c.B, H=c.H, W=c.W, src=src, w=wp, cout=64, ks=1, out=out, out_ctot=octot, out_coff=ocoff,
                    shift=blk.confusion.bias.detach(), relu=1, res=X, nsplit=nsc, w_amax=wis,
                    out_amax=am_o)
        s.Y = Act(out, octot, ocoff, 64, amax=am_o)
        return s

    def _res_fwd(self, c, rb, F0: Act, out, octot, ocoff, am_o, new_amax, buf):
        """One ResBlock (reference model/tactileSR_model.py:222-225): relu(x + conv2(relu(conv1(x))))."""
        s = _Ctx()
        s.X = F0
        s.f1 = buf(64)
        s.F1 = Act(s.f1, 64, 0, 64, amax=new_amax())
        src1, w1, wis1, ns1 = self._form(c, rb.conv1, F0)
        src2, w2, wis2, ns2 = self._form(c, rb.conv2, s.F1)
        with _timed(self.profile, ("fwd", 3, 64, 64)):
            conv_ex(B=c.B, H=c.H, W=c.W, src=src1, w=w1, cout=64, ks=3, out=s.f1, out_ctot=64, out_coff=0,
                    shift=rb.conv1.bias.detach(), relu=1, nsplit=ns1, w_amax=wis1, out_amax=s.F1.amax)
            conv_ex(B=c.B, H=c.H, W=c.W, src=src2, w=w2, cout=64, ks=3, out=out, out_ctot=octot,
                    out_coff=ocoff, shift=rb.conv2.bias.detach(), relu=1, res=F0, nsplit=ns2,
                    w_amax=wis2, out_amax=am_o)
        s.Y = Act(out, octot, ocoff, 64, amax=am_o)
        return s

    # ------------------------------------------------------------------ forward
    def forward(self, x: torch.Tensor):
        m = self.m
        dev = x.device
        B, hin, win = x.shape[0], x.shape[2], x.shape[3]
        sf, T, A = m.scale_factor, m.seqsCnt, m.axisCnt
        H, W = hin * sf, win * sf
        HW = H * W
        # every refusal comes before the first launch: a refused step leaves parameters and statistics as they were
        m._check_input(x)
        check_trainable_size(H, W)
        if len(m.patternFeatureExtra_layer) == 0:
            raise _lib.TactileSRHipError("train path needs patternFeatureExtraLayerCnt >= 1")
        if len(m.forceFeatureExtra_layer) == 0:
            raise _lib.TactileSRHipError("train path needs forceFeatureExtraLayerCnt >= 1")
        c = self._new_ctx(B, H, W, dev)
        c.x, c.hin, c.win = x.detach(), hin, win
        c.want_dx = False        # TrainFn sets it when the taxels require grad: backward then also leaves c.dx
        c.want = self._want_default(m.named_parameters())      # (TrainFn: what autograd asks for instead)
        st_entries = c.st_entries

        def buf(ch):
            return torch.empty(B * ch * HW, dtype=self.act_dtype, device=dev)

        self._weight_scales(c)
        new_amax = self._amax_pool(dev)
        ctot_in = x.shape[1]
        # ---- pattern stems
        c.z1, c.bn1, c.am_z1 = [], [], []
        c.catT = buf(64 * T)
        c.am_catT = new_amax()
        c.bn2 = torch.empty(4, 64 * T, dtype=torch.float32, device=dev)
        for t, seq in enumerate(m.inputLayer_pattern_list):
            z1 = buf(64)
            am = new_amax()
            self._stem(x, ctot_in, A * t, A, hin, win, sf, seq[1].weight.detach(), z1, 0, B, am)
            if seq[2].training:
                self._twin("tsr_cb16_stats", ptr(z1), _I(64), _I(0), _I(B), _I(HW), ptr(c.slab), ptr(c.slab_cnt))
                v1 = self._bn_finalize(c, None, seq[2], c.slab, c.slab_cnt, st_entries, 64)
            else:
                v1 = self._bn_held_vec(None, seq[2], 64)
            c.z1.append(z1)
            c.bn1.append(v1)
            c.am_z1.append(am)
            v2 = self._conv_bn(c, Act(z1, 64, 0, 64, v1[0], v1[1], amax=am), seq[4], seq[5], c.catT, 64 * T, 64 * t,
                               out_amax=c.am_catT)
            c.bn2[:, 64 * t:64 * (t + 1)] = v2
        # ---- fuse conv
        c.zf = buf(64)
        am_zf = new_amax()
        c.bnf = self._conv_bn(c, Act(c.catT, 64 * T, 0, 64 * T, c.bn2[0], c.bn2[1], amax=c.am_catT),
                              m.inputContact_layer[0], m.inputContact_layer[1], c.zf, 64, 0, out_amax=am_zf)
        X = Act(c.zf, 64, 0, 64, c.bnf[0], c.bnf[1], c.bnf[2], c.bnf[3], amax=am_zf)
        # ---- MSRB chain
        c.hcat = buf(128)
        c.am_hcat = new_amax()
        c.blocks = []
        n_msrb = len(m.patternFeatureExtra_layer)
        for i, blk in enumerate(m.patternFeatureExtra_layer):
            if i == n_msrb - 1:
                out, octot, ocoff, am_o = c.hcat, 128, 64, c.am_hcat
            else:
                out, octot, ocoff, am_o = buf(64), 64, 0, new_amax()
            s = self._msrb_fwd(c, blk, X, out, octot, ocoff, am_o, new_amax, buf)
            X = s.Y
            c.blocks.append(s)
        # ---- force branch
        c.f0 = buf(64)
        am_f0 = new_amax()
        self._stem(x, ctot_in, 0, A, hin, win, sf, m.input_layer_force[1].weight.detach(), c.f0, 1, B, am_f0)
        F0 = Act(c.f0, 64, 0, 64, amax=am_f0)
        c.res = []
        n_res = len(m.forceFeatureExtra_layer)
        for i, rb in enumerate(m.forceFeatureExtra_layer):
            if i == n_res - 1:
                out, octot, ocoff, am_o = c.hcat, 128, 0, c.am_hcat
            else:
                out, octot, ocoff, am_o = buf(64), 64, 0, new_amax()
            s = self._res_fwd(c, rb, F0, out, octot, ocoff, am_o, new_amax, buf)
            F0 = s.Y
            c.res.append(s)
        # ---- head
        c.h0 = buf(128)
        HC, wh, wish, nsh = self._form(c, m.output_layer[0], Act(c.hcat, 128, 0, 128, amax=c.am_hcat))
        conv_ex(B=B, H=H, W=W, src=HC, w=wh, cout=128, ks=3, out=c.h0, out_ctot=128, out_coff=0, relu=1, nsplit=nsh,
                w_amax=wish)
        out = torch.empty(B, 1, H, W, dtype=torch.float32, device=dev)
        self._twin("tsr_head_fwd", ptr(c.h0), _I(128), _I(128), ptr(m.output_layer[2].weight.detach()), ptr(out), _I(1),
                   _I(B), _I(H), _I(W))
        c.out = out
        self._bump_nbt(c)
        self.last_ctx = c if self.keep_ctx else None
        return out, c

    @torch.no_grad()
    def activation_masks(self, c: _Ctx, img0: int = 0, nimg: int = None):
        """The ReLU activation pattern this forward took for images [img0, img0+nimg) (default: all), as
        {name: bool (nimg,C,H,W) tensor} keyed like the CPU
        oracle's ``ReluTap`` (test plumbing: the parity tests evaluate the fp64 gradient on exactly this pattern).
        BN layers store the raw conv output z plus per-channel (scale, shift); every kernel evaluates
        ``fmaf(z, scale, shift) > 0``, whose sign equals that of the exactly evaluated z*scale+shift in fp64."""
        m = self.m
        H, W = c.H, c.W
        B = c.B - img0 if nimg is None else nimg
        assert 0 <= img0 and B > 0 and img0 + B <= c.B

        def sub(buf, ctot):          # CB16 is image-major: a batch slice is a contiguous range
            return buf[img0 * ctot * H * W:(img0 + B) * ctot * H * W]

        def bn_mask(buf, ctot, coff, C, scale, shift):
            z = from_cb16(sub(buf, ctot), B, C, H, W, ctot, coff).double()
            return (z * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)) > 0

        def pos(a: Act):
            return from_cb16(sub(a.buf, a.ctot), B, a.c, H, W, a.ctot, a.coff) > 0

        out = {}
        T = m.seqsCnt
        for t in range(T):
            v1 = c.bn1[t]
            out[f"inputLayer_pattern_list.{t}.2"] = bn_mask(c.z1[t], 64, 0, 64, v1[0], v1[1])
            o = 64 * t
            out[f"inputLayer_pattern_list.{t}.5"] = bn_mask(c.catT, 64 * T, o, 64, c.bn2[0, o:o + 64], c.bn2[1, o:o + 64])
        out["inputContact_layer.1"] = bn_mask(c.zf, 64, 0, 64, c.bnf[0], c.bnf[1])
        for i, s in enumerate(c.blocks):
            pre = f"patternFeatureExtra_layer.{i}"
            out[pre + ".conv_3_1.1"] = bn_mask(s.cat1, 128, 0, 64, s.bn_c1[0, :64], s.bn_c1[1, :64])
            out[pre + ".conv_5_1.1"] = bn_mask(s.cat1, 128, 64, 64, s.bn_c1[0, 64:], s.bn_c1[1, 64:])
            out[pre + ".conv_3_2.1"] = bn_mask(s.cat2, 256, 0, 128, s.bn_c2[0, :128], s.bn_c2[1, :128])
            out[pre + ".conv_5_2.1"] = bn_mask(s.cat2, 256, 128, 128, s.bn_c2[0, 128:], s.bn_c2[1, 128:])
            out[pre + ".out"] = pos(s.Y)
        out["force_in"] = pos(Act(c.f0, 64, 0, 64))
        for i, s in enumerate(c.res):
            pre = f"forceFeatureExtra_layer.{i}"
            out[pre + ".conv1"] = pos(s.F1)
            out[pre + ".out"] = pos(s.Y)
        out["head0"] = pos(Act(c.h0, 128, 0, 128))
        out["out"] = c.out[img0:img0 + B] > 0
        return out

    # ------------------------------------------------------------------ backward pieces
    def _nsplit(self, B, tiles, ks, cout, cin):
        """Batch splits of the wgrad launch: slices*nsplit ~ 2 x (3 workgroups x 256 CUs) resident slots;
        work items are (image, 8x8 patch) pairs, so splits may outnumber images."""
        slices = ks * (cout // 64) * (cin // 64)
        return max(1, min(B * tiles, (1024 if self.nsplit else 1536) // slices))   # 2 (16-bit) / 3 (f32) WGs per CU

    def _wgrad(self, c, a: Act, dz: Act, conv, grads, name, with_bias):
        """The weight-gradient launch of `conv` (plan record ("wgrad", name)): it runs whole when its weight or its bias
        gradient is wanted; only the wanted ones are reduced out of the split slabs and handed to `grads`."""
        if ("wgrad", name) not in c.live:
            return
        w = conv.weight
        cout, cin, ks = w.shape[0], w.shape[1], w.shape[2]
        if self.io16 and _lib.load().tsr_conv2d_wgrad_b16k(cout, cin, ks):
            a = self._plain(c, a)      # the LDS-DMA weight-gradient kernel takes its operands as they are stored
        if self.nsplit:       # 16-bit MFMA form: the library sizes the batch split for its tile shape
            ns = _lib.load().tsr_conv2d_wgrad_splits(cout, cin, ks, self.nsplit, c.B, c.H, c.W)
        else:
            ns = self._nsplit(c.B, ((c.H + 7) // 8) * ((c.W + 7) // 8), ks, cout, cin)
        n = cout * cin * ks * ks
        slab = torch.empty(ns * n, dtype=torch.float32, device=w.device)
        bslab = torch.empty(ns * cout, dtype=torch.float32, device=w.device) if with_bias else None
        with _timed(self.profile, ("wgrad", ks, cout, cin)):
            if self.nsplit:
                call("tsr_conv2d_wgrad_bf16s", ptr(a.buf), _I(a.ctot), _I(a.coff), _I(cin), ptr(a.scale), ptr(a.shift),
                     ptr(dz.buf), _I(dz.ctot), _I(dz.coff), _I(cout), _I(ks), _I(self.nsplit), ptr(a.amax),
                     ptr(dz.amax), ptr(slab), ptr(bslab), _I(ns), _I(c.B), _I(c.H), _I(c.W), stream())
            else:
                call("tsr_conv2d_wgrad", ptr(a.buf), _I(a.ctot), _I(a.coff), _I(cin), ptr(a.scale), ptr(a.shift),
                     ptr(dz.buf), _I(dz.ctot), _I(dz.coff), _I(cout), _I(ks), ptr(slab), ptr(bslab), _I(ns),
                     _I(c.B), _I(c.H), _I(c.W), stream())
        if name + ".weight" in c.want:
            gw = grads.dest(name + ".weight", w.shape)
            call("tsr_reduce_splits", ptr(slab), ptr(gw), _L(n), _I(ns), _F(1.0), stream())
            grads.put(name + ".weight", gw)
        if with_bias and name + ".bias" in c.want:
            gb = grads.dest(name + ".bias", (cout,))
            call("tsr_reduce_splits", ptr(bslab), ptr(gb), _L(cout), _I(ns), _F(1.0), stream())
            grads.put(name + ".bias", gb)

    def _dgrad(self, c, dz: Act, conv, ci0, nprime, out, out_ctot, out_coff, res: Act = None, mask: Act = None,
               bn=False, out_amax=None):
        """d(input)[ci0:ci0+nprime] of conv given dz; optional + res, ReLU mask, BN-backward sums.  Returns the statistics-slab
        entries of the launch: what a following `_bn_bwd` reduces."""
        cout, ks = conv.weight.shape[0], conv.weight.shape[2]
        # bf16 storage: the 128-channel 3x3 / 5x5 dgrads (masked or not) run conv_b16k
        plain = dz.scale is None and (res is None or res.scale is None) and (ks > 1 or (mask is not None and res is None))
        dz, wp, wa, ns = self._form(c, conv, dz, dgrad=(ci0, nprime, plain))
        with _timed(self.profile, ("dgrad", ks, nprime, cout)):
            conv_ex(B=c.B, H=c.H, W=c.W, src=dz, w=wp, cout=nprime, ks=ks, out=out, out_ctot=out_ctot,
                    out_coff=out_coff, res=res, epi_mode=2 if mask is not None else 0, mask=mask, bn=bn,
                    slab=c.slab if bn else None, slab_cnt=None, nsplit=ns, w_amax=wa,
                    out_amax=out_amax)
        return self._entries(c, nprime, ks, ns)

    def _bn_bwd(self, c, layer, g_buf, g_ctot, g_coff, z: Act, zoff, C, bn_vec, grads, entries, out_amax=None, gnames=None):
        """Finish BatchNorm backward for C channels whose masked gradient g sits in g_buf (slab sums, `entries` of them,
        were just produced by the dgrad epilogue over the same C channels).  `gnames` = (weight, bias) parameter names:
        the wanted ones of dgamma / dbeta are then written straight into their gradient slots (no copy launches).
        Plan records ("bn_bwd_finalize", layer) -- needed for dgamma / dbeta or for the apply pass -- and
        ("bn_bwd_apply", layer), which turns g into dz in place and runs only when dz is consumed.
        A layer in eval mode (`c.bn_eval`): dz = scale * g -- one pass over g alone (tsr_bn_bwd_apply_eval), and the finalize
        (tsr_bn_bwd_finalize_eval: dgamma, dbeta only) runs just when one of the two is wanted."""
        finalize = ("bn_bwd_finalize", layer) in c.live
        held = bn_held(layer, c.bn_eval)
        if not finalize and not (held and ("bn_bwd_apply", layer) in c.live):
            return None
        dev = g_buf.device
        out = torch.empty(5, C, dtype=torch.float32, device=dev)
        gnames = tuple(n if n in c.want else None for n in gnames) if gnames else (None, None)
        dg = grads.dest(gnames[0], (C,)) if gnames[0] else out[0]
        db = grads.dest(gnames[1], (C,)) if gnames[1] else out[1]
        if held:
            if finalize:
                call("tsr_bn_bwd_finalize_eval", ptr(c.slab), _I(entries), _I(C), ptr(dg), ptr(db), ptr(c.work), stream())
        else:
            call("tsr_bn_bwd_finalize", ptr(c.slab), _I(entries), _I(C), _D(float(c.B * c.HW)),
                 ptr(bn_vec[0]), ptr(bn_vec[2]), ptr(bn_vec[3]), ptr(dg), ptr(db), ptr(out[2]), ptr(out[3]),
                 ptr(out[4]), ptr(c.work), stream())
            # layers that share this launch, one of them in eval mode (a mixed stage-1 pair): dgamma / dbeta are the same sums
            # in both modes and c1 = scale already; without the batch-statistics terms its channels get dz = scale * g
            for k, n in enumerate(bn_members(layer)):
                if n in c.bn_eval:
                    w = C // len(bn_members(layer))
                    out[3:5, k * w:(k + 1) * w].zero_()
        if finalize and gnames[0]:
            grads.put(gnames[0], dg)
        if finalize and gnames[1]:
            grads.put(gnames[1], db)
        if ("bn_bwd_apply", layer) not in c.live:
            return out if finalize else None
        if held:
            self._twin("tsr_bn_bwd_apply_eval", ptr(g_buf), _I(g_ctot), _I(g_coff), ptr(bn_vec[0]), _I(C), _I(c.B), _I(c.HW),
                       amax=(out_amax,))
            return out if finalize else None
        self._twin("tsr_bn_bwd_apply", ptr(g_buf), _I(g_ctot), _I(g_coff), ptr(z.buf), _I(z.ctot), _I(z.coff + zoff),
                   ptr(out[2]), ptr(out[3]), ptr(out[4]), _I(C), _I(c.B), _I(c.HW), amax=(out_amax,))
        return out   # rows 0,1 = dgamma, dbeta

    def _res_bwd(self, c, s, rb, name, dpre: Act, grads, new_amax, buf, mask_input=True):
        """Backward of one ResBlock.  `dpre` = gradient w.r.t. the block output BEFORE its ReLU; returns the gradient
        w.r.t. the block input (None when the backward plan has no launch producing it) -- masked by the input's own ReLU
        pattern (`mask_input`, the chained engine: the input is the previous block's post-ReLU output) or plain (standalone
        module)."""
        name = name + "." if name else ""          # (standalone module: parameter names carry no prefix)
        F1 = s.F1
        self._wgrad(c, F1, dpre, rb.conv2, grads, name + "conv2", True)
        if ("dgrad", name + "conv2") not in c.live:      # nothing below conv2 wants a gradient
            return None
        d1 = buf(64)
        D1 = Act(d1, 64, 0, 64, amax=new_amax())
        self._dgrad(c, dpre, rb.conv2, 0, 64, d1, 64, 0, mask=F1, out_amax=D1.amax)
        self._wgrad(c, s.X, D1, rb.conv1, grads, name + "conv1", True)
        if ("dgrad", name + "conv1") not in c.live:
            return None
        d0 = buf(64)
        am = new_amax()
        self._dgrad(c, D1, rb.conv1, 0, 64, d0, 64, 0, res=dpre, mask=s.X if mask_input else None, out_amax=am)
        return Act(d0, 64, 0, 64, amax=am)

    def _msrb_bwd(self, c, s, blk, name, dpre: Act, grads, new_amax, buf, tag="msrb", mask_input=True, in_bn=None):
        """Backward of one MSRB.  `dpre` = gradient w.r.t. the block output BEFORE its ReLU; returns the gradient w.r.t.
        the block input (None when the backward plan has no launch producing it): masked by the input's ReLU pattern / with
        the BatchNorm-backward sums of a virtual input (`mask_input`, the chained engine; `in_bn`: that BatchNorm's path) or
        plain (standalone module) -- and the statistics-slab entries of those sums, for the `_bn_bwd` of `in_bn`."""
        name = name + "." if name else ""          # (standalone module: parameter names carry no prefix)
        on = lambda kind, layer: (kind, name + layer) in c.live
        sums = lambda layer: on("bn_bwd_finalize", layer)      # whether the dgrad in front of this BatchNorm leaves its sums
        # confusion 1x1: a = relu(bn(cat2)), dz = dpre
        self._wgrad(c, s.A2, dpre, blk.confusion, grads, name + "confusion", True)
        if not (on("dgrad", "confusion[0:128]") or on("dgrad", "confusion[128:256]")):
            return None, None
        g2 = buf(256)
        am_g2 = [new_amax(), new_amax()]
        for half, nm in enumerate(("conv_3_2", "conv_5_2")):
            o = 128 * half
            if not on("dgrad", f"confusion[{o}:{o + 128}]"):
                continue
            mk = Act(s.cat2, 256, o, 128, s.bn_c2[0, o:o + 128], s.bn_c2[1, o:o + 128], s.bn_c2[2, o:o + 128],
                     s.bn_c2[3, o:o + 128])
            e = self._dgrad(c, dpre, blk.confusion, o, 128, g2, 256, o, mask=mk, bn=sums(nm + ".1"))
            self._bn_bwd(c, f"{name}{nm}.1", g2, 256, o, Act(s.cat2, 256, 0, 256), o, 128, s.bn_c2[:, o:o + 128], grads, e,
                         out_amax=am_g2[half], gnames=(f"{name}{nm}.1.weight", f"{name}{nm}.1.bias"))
        if self.debug is not None:
            self.debug[f"{tag}.dz2"] = g2.clone()
        DZ32, DZ52 = Act(g2, 256, 0, 128, amax=am_g2[0]), Act(g2, 256, 128, 128, amax=am_g2[1])
        self._wgrad(c, s.A1, DZ32, blk.conv_3_2[0], grads, f"{name}conv_3_2.0", True)
        self._wgrad(c, s.A1, DZ52, blk.conv_5_2[0], grads, f"{name}conv_5_2.0", True)
        if not on("dgrad", "conv_5_2.0"):          # (the two stage-2 dgrads fill one tensor: both are planned or neither)
            return None, None
        g1 = buf(128)
        self._dgrad(c, DZ32, blk.conv_3_2[0], 0, 128, g1, 128, 0)
        mk = Act(s.cat1, 128, 0, 128, s.bn_c1[0], s.bn_c1[1], s.bn_c1[2], s.bn_c1[3])
        e = self._dgrad(c, DZ52, blk.conv_5_2[0], 0, 128, g1, 128, 0, res=Act(g1, 128, 0, 128), mask=mk,
                        bn=sums("conv_3_1.1|conv_5_1.1"))
        am_g1 = new_amax()
        r = self._bn_bwd(c, f"{name}conv_3_1.1|conv_5_1.1", g1, 128, 0, Act(s.cat1, 128, 0, 128), 0, 128, s.bn_c1, grads, e,
                         out_amax=am_g1)
        for gname, row, lo in ((f"{name}conv_3_1.1.weight", 0, 0), (f"{name}conv_3_1.1.bias", 1, 0),
                               (f"{name}conv_5_1.1.weight", 0, 64), (f"{name}conv_5_1.1.bias", 1, 64)):
            if gname in c.want:
                grads.put_copy(gname, r[row, lo:lo + 64])
        del g2
        if self.debug is not None:
            self.debug[f"{tag}.dz1"] = g1.clone()
        DZ31, DZ51 = Act(g1, 128, 0, 64, amax=am_g1), Act(g1, 128, 64, 64, amax=am_g1)
        self._wgrad(c, s.X, DZ31, blk.conv_3_1[0], grads, f"{name}conv_3_1.0", True)
        self._wgrad(c, s.X, DZ51, blk.conv_5_1[0], grads, f"{name}conv_5_1.0", True)
        if not on("dgrad", "conv_5_1.0"):          # (likewise one tensor: dx)
            return None, None
        dx = buf(64)
        self._dgrad(c, DZ31, blk.conv_3_1[0], 0, 64, dx, 64, 0, res=dpre)
        virtual = mask_input and s.X.scale is not None
        am = new_amax()
        e = self._dgrad(c, DZ51, blk.conv_5_1[0], 0, 64, dx, 64, 0, res=Act(dx, 64, 0, 64),
                        mask=s.X if mask_input else None, bn=virtual and ("bn_bwd_finalize", in_bn) in c.live,
                        out_amax=None if virtual else am)
        return Act(dx, 64, 0, 64, amax=am), e

    # ------------------------------------------------------------------ backward
    def _want_default(self, named):
        """The want-set of a forward that autograd did not record (the engine driven directly): `requires_grad`."""
        return frozenset(n for n, p in named if p.requires_grad)

    def backward(self, c: _Ctx, dout: torch.Tensor):
        m = self.m
        dev = dout.device
        B, H, W, HW = c.B, c.H, c.W, c.HW
        from ..ddp import GradSink
        T = m.seqsCnt
        # the launches something that wants a gradient depends on (all of today's list when every parameter is trainable)
        c.live = {r.key for r in backward_plan(T, len(c.blocks), len(c.res), c.want, c.want_dx, c.bn_eval)}
        on = lambda kind, layer: (kind, layer) in c.live
        grads = GradSink(self, dict(m.named_parameters()), dev, token=c, want=c.want)

        def buf(ch):
            return torch.empty(B * ch * HW, dtype=self.act_dtype, device=dev)

        new_amax = self._amax_pool(dev)      # a gradient tensor consumed by an MFMA launch carries max|.|
        dout = dout.contiguous().float()
        # taxel gradient (only when the input requires grad): frame 0 gets the force stem's store, then its pattern stem's add
        dx = torch.empty(c.x.shape, dtype=torch.float32, device=dev) if c.want_dx else None
        c.dx = dx
        if not c.live:
            return grads.finalize()
        # ---- head: out = relu(conv(h0)), h0 = relu(conv(hcat))
        dz_h0 = buf(128)
        am_dzh0 = new_amax()
        if on("head_bwd", "output_layer.2"):
            ns = max(1, min(B * (8 if H > 64 else 1), 2048))     # (image split, row band) entries: ~8 resident workgroups per CU
            wslab = torch.empty(ns * 128 * 9, dtype=torch.float32, device=dev)
            self._twin("tsr_head_bwd", ptr(dout), ptr(c.out), ptr(c.h0), _I(128), _I(128),
                       ptr(m.output_layer[2].weight.detach()), ptr(dz_h0), _I(128), ptr(wslab), _I(ns), _I(B), _I(H), _I(W),
                       amax=(am_dzh0,))
            gw = grads.dest("output_layer.2.weight", m.output_layer[2].weight.shape)
            call("tsr_reduce_splits", ptr(wslab), ptr(gw), _L(128 * 9), _I(ns), _F(1.0), stream())
            grads.put("output_layer.2.weight", gw)
        else:       # ("head_dgrad", "output_layer.2"): the head weight is frozen, dz_h0 is still consumed
            self._twin("tsr_head_dgrad", ptr(dout), ptr(c.out), ptr(c.h0), _I(128), _I(128),
                       ptr(m.output_layer[2].weight.detach()), ptr(dz_h0), _I(128), _I(B), _I(H), _I(W), amax=(am_dzh0,))
        DZ = Act(dz_h0, 128, 0, 128, amax=am_dzh0)
        HC = Act(c.hcat, 128, 0, 128, amax=c.am_hcat)
        self._wgrad(c, HC, DZ, m.output_layer[0], grads, "output_layer.0", False)
        if not on("dgrad", "output_layer.0"):          # only the head trains
            return grads.finalize()
        g_hcat = buf(128)
        am_ghcat = new_amax()
        self._dgrad(c, DZ, m.output_layer[0], 0, 128, g_hcat, 128, 0, mask=HC, out_amax=am_ghcat)
        if self.debug is not None:
            self.debug["dz_h0"] = dz_h0.clone()
            self.debug["g_hcat"] = g_hcat.clone()
        del dz_h0

        # ---- force branch (ResBlocks, reversed); gradient w.r.t. block output pre-ReLU in `dpre`
        dpre = Act(g_hcat, 128, 0, 64, amax=am_ghcat)
        for i in reversed(range(len(c.res))):
            if dpre is not None:
                dpre = self._res_bwd(c, c.res[i], m.forceFeatureExtra_layer[i], f"forceFeatureExtra_layer.{i}", dpre, grads,
                                     new_amax, buf)
        if on("stem_wgrad", "input_layer_force.1"):
            ns = max(1, min(B, 2048))     # image splits: ~8 resident workgroups per CU hide the load latency
            self._stem_wgrad(c, "input_layer_force.1.weight", m.input_layer_force[1].weight, 0, dpre.buf, dpre.ctot, dpre.coff,
                             ns, grads)
        if on("stem_dgrad", "input_layer_force.1"):
            self._stem_dgrad(c, m.input_layer_force[1].weight, dpre.buf, dpre.ctot, dpre.coff, dx, 0, 0)

        # ---- pattern branch: MSRB blocks reversed
        dpre = Act(g_hcat, 128, 64, 64, amax=am_ghcat)
        for i in reversed(range(len(c.blocks))):
            if dpre is not None:
                dpre, e = self._msrb_bwd(c, c.blocks[i], m.patternFeatureExtra_layer[i], f"patternFeatureExtra_layer.{i}", dpre,
                                         grads, new_amax, buf, tag=f"msrb{i}", in_bn="inputContact_layer.1")
        if dpre is None:          # nothing at or below the first MSRB's input wants a gradient
            return grads.finalize()
        # X of block 0 is the fuse conv's relu(bn(zf)): finish its BN backward -> dzf
        self._bn_bwd(c, "inputContact_layer.1", dpre.buf, 64, 0, Act(c.zf, 64, 0, 64), 0, 64, c.bnf, grads, e,
                     out_amax=dpre.amax, gnames=("inputContact_layer.1.weight", "inputContact_layer.1.bias"))
        AT = Act(c.catT, 64 * T, 0, 64 * T, c.bn2[0], c.bn2[1], c.bn2[2], c.bn2[3], amax=c.am_catT)
        self._wgrad(c, AT, dpre, m.inputContact_layer[0], grads, "inputContact_layer.0", False)
        gT = buf(64 * T)
        for t, seq in enumerate(m.inputLayer_pattern_list):
            name = f"inputLayer_pattern_list.{t}"
            o = 64 * t
            if not on("dgrad", f"inputContact_layer.0[{o}:{o + 64}]"):
                continue
            mk = Act(c.catT, 64 * T, o, 64, c.bn2[0, o:o + 64], c.bn2[1, o:o + 64], c.bn2[2, o:o + 64],
                     c.bn2[3, o:o + 64])
            e = self._dgrad(c, dpre, m.inputContact_layer[0], o, 64, gT, 64 * T, o, mask=mk,
                            bn=on("bn_bwd_finalize", name + ".5"))
            am_gT = new_amax()
            self._bn_bwd(c, name + ".5", gT, 64 * T, o, Act(c.catT, 64 * T, 0, 64 * T), o, 64, c.bn2[:, o:o + 64], grads, e,
                         out_amax=am_gT, gnames=(name + ".5.weight", name + ".5.bias"))
            DZ2 = Act(gT, 64 * T, o, 64, amax=am_gT)
            v1 = c.bn1[t]
            A1 = Act(c.z1[t], 64, 0, 64, v1[0], v1[1], v1[2], v1[3], amax=c.am_z1[t])
            self._wgrad(c, A1, DZ2, seq[4], grads, name + ".4", False)
            if not on("dgrad", name + ".4"):
                continue
            g1 = buf(64)
            e = self._dgrad(c, DZ2, seq[4], 0, 64, g1, 64, 0, mask=A1, bn=on("bn_bwd_finalize", name + ".2"))
            self._bn_bwd(c, name + ".2", g1, 64, 0, Act(c.z1[t], 64, 0, 64), 0, 64, v1, grads, e,
                         gnames=(name + ".2.weight", name + ".2.bias"))
            if on("stem_wgrad", name + ".1"):
                ns = max(1, min(B * (8 if H > 64 else 1), 2048))     # (image split, row band) entries
                self._stem_wgrad(c, name + ".1.weight", seq[1].weight, m.axisCnt * t, g1, 64, 0, ns, grads)
            if on("stem_dgrad", name + ".1"):
                self._stem_dgrad(c, seq[1].weight, g1, 64, 0, dx, m.axisCnt * t, int(t == 0))
        return grads.finalize()

    def _stem_wgrad(self, c, gname, weight, x_coff, dz, dz_ctot, dz_coff, ns, grads):
        """The weight gradient `gname` of one stem (bilinear x sf + conv 3 -> 64 on taxel channels [x_coff, x_coff + 3)) given
        its dz: `ns` split slabs, reduced into the gradient's slot."""
        sslab = torch.empty(ns * 64 * 27, dtype=torch.float32, device=dz.device)
        self._twin("tsr_stem_wgrad", ptr(c.x), _I(c.x.shape[1]), _I(x_coff), _I(c.hin), _I(c.win), _I(self.m.scale_factor),
                   ptr(dz), _I(dz_ctot), _I(dz_coff), ptr(sslab), _I(ns), _I(c.B))
        gw = grads.dest(gname, weight.shape)
        call("tsr_reduce_splits", ptr(sslab), ptr(gw), _L(64 * 27), _I(ns), _F(1.0), stream())
        grads.put(gname, gw)

    def _stem_dgrad(self, c, weight, dz, dz_ctot, dz_coff, dx, dx_coff, accumulate):
        """dx[:, dx_coff:dx_coff+3] (=|+=) the taxel gradient of one stem (bilinear x sf + conv 3 -> 64) given its dz."""
        self._twin("tsr_stem_dgrad", ptr(weight.detach().contiguous()), ptr(dz), _I(dz_ctot), _I(dz_coff), _I(c.hin),
                   _I(c.win), _I(self.m.scale_factor), ptr(dx), _I(dx.shape[1]), _I(dx_coff), _I(accumulate), _I(c.B))


class TrainFn(torch.autograd.Function):
    """out = engine.forward(x; params) of a ``TrainEngine`` (the whole network) or a ``BlockEngine`` (a standalone MSRB /
    ResBlock); gradients for x and the parameters.  ``params`` are passed only so that autograd
    routes their gradients; the engine reads them from the module."""

    @staticmethod
    def forward(ctx, engine: TrainEngine, names, x, *params):
        out, c = engine.forward(x)
        c.want_dx = bool(ctx.needs_input_grad[2])      # the input's gradient only when the caller's input requires grad
        c.want = frozenset(n for n, need in zip(names, ctx.needs_input_grad[3:]) if need)      # one flag per parameter
        ctx.engine, ctx.c, ctx.names = engine, c, names
        if any(ctx.needs_input_grad):
            from ..ddp import note_forward
            note_forward(engine, c)          # the arena is handed out only to the sole outstanding application
        return out

    @staticmethod
    def backward(ctx, dout):
        c = ctx.c
        if c is None:
            # the first backward released the forward's context (activations, BatchNorm vectors: device memory of the size
            # of the step) -- a second pass over the same graph has nothing to differentiate
            raise _lib.TactileSRHipError(
                "second backward through the same tactilesr_amd forward: the first backward released the saved "
                "activations (retain_graph=True does not keep them); run the forward again for another backward")
        grads = ctx.engine.backward(c, dout)
        dx, c.dx = c.dx, None
        ctx.c = None
        missing = [n for n in ctx.names if n in c.want and n not in grads]
        if missing:
            raise _lib.TactileSRHipError(f"backward produced no gradient for {missing[:4]}...")
        return (None, None, dx) + tuple(grads.get(n) if n in c.want else None for n in ctx.names)


class BlockEngine(TrainEngine):
    """Train-mode forward / backward of ONE standalone ``MSRB`` or ``ResBlock`` module on an NCHW tensor (reference
    model/tactileSR_model.py:196-206,222-225 are callable modules): the same kernels and the same per-block code as the
    whole-network engine, with NCHW <-> CB16 conversion at the boundary and the gradient w.r.t. the block input
    left unmasked, as NCHW, on the context's `dx`."""

    def __init__(self, block, kind: str, impl: str = "fp16x3"):
        super().__init__(None, impl)
        assert kind in ("msrb", "res")
        self.block, self.kind = block, kind

    def _mfma_convs(self):
        b = self.block
        if self.kind == "msrb":
            return [b.conv_3_1[0], b.conv_5_1[0], b.conv_3_2[0], b.conv_5_2[0], b.confusion]
        return [b.conv1, b.conv2]

    def _amax_slots(self):
        return 64

    def forward(self, x: torch.Tensor):
        B, C, H, W = x.shape
        dev = x.device
        c = self._new_ctx(B, H, W, dev)
        c.want = self._want_default(self.block.named_parameters())      # (TrainFn: what autograd asks for instead)
        c.want_dx = True
        self._weight_scales(c)
        new_amax = self._amax_pool(dev)

        def buf(ch):
            return torch.empty(B * ch * H * W, dtype=self.act_dtype, device=dev)

        am_x = new_amax()
        if am_x is not None:
            am_x.copy_(x.abs().amax())          # device-side: the operand scale of the first convs
        X = Act(to_cb16(x).to(self.act_dtype), 64, 0, 64, amax=am_x)
        out, am_o = buf(64), new_amax()
        fwd = self._msrb_fwd if self.kind == "msrb" else self._res_fwd
        c.s = fwd(c, self.block, X, out, 64, 0, am_o, new_amax, buf)
        self._bump_nbt(c)
        self.last_ctx = c if self.keep_ctx else None
        return from_cb16(out, B, 64, H, W), c

    def backward(self, c: _Ctx, dout: torch.Tensor):
        from ..ddp import GradSink
        dev = dout.device
        B, H, W = c.B, c.H, c.W
        c.live = {r.key for r in block_backward_plan(self.kind, c.want, c.want_dx, c.bn_eval)}
        grads = GradSink(self, dict(self.block.named_parameters()), dev, token=c, want=c.want)
        c.dx = None
        if not c.live:
            return grads.finalize()
        new_amax = self._amax_pool(dev)

        def buf(ch):
            return torch.empty(B * ch * H * W, dtype=self.act_dtype, device=dev)

        # gradient w.r.t. the block output BEFORE its ReLU (in the whole-network engine the consumer's dgrad epilogue
        # applies this mask; here it is one elementwise pass over the boundary tensor)
        d = (to_cb16(dout.contiguous().float()) * (c.s.Y.buf > 0)).to(self.act_dtype)
        am = new_amax()
        if am is not None:
            am.copy_(d.abs().amax())
        dpre = Act(d, 64, 0, 64, amax=am)
        if self.kind == "msrb":
            dx, _ = self._msrb_bwd(c, c.s, self.block, "", dpre, grads, new_amax, buf, mask_input=False)
        else:
            dx = self._res_bwd(c, c.s, self.block, "", dpre, grads, new_amax, buf, mask_input=False)
        if dx is not None:
            c.dx = from_cb16(dx.buf, B, 64, H, W)
        return grads.finalize()
