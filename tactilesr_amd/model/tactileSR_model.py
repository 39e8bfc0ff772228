"""MI355X-native drop-in for the reference's ``model/tactileSR_model.py``.

Same public surface as the reference classes -- ``TactileSR(scale_factor, seqsCnt,
axisCnt, patternFeatureExtraLayerCnt, forceFeatureExtraLayerCnt)``, ``MSRB``,
``ResBlock``; same attribute names, submodule names, ``state_dict`` keys (205 for
T=1) and construction-time RNG consumption (so ``torch.manual_seed(s); TactileSR()``
yields bit-identical initial weights; /root/reference/model/tactileSR_model.py:22-65,
92-98,161-194,217-220) -- but ``forward`` never touches ATen convolution: it drives
the hand-written HIP kernels of ``libtactilesr_hip.so`` through the C ABI of
``include/tactilesr_hip.h``.  The nn.Conv2d / nn.BatchNorm2d children are parameter
containers only.  There is no CPU fallback: CPU tensors or a missing library raise.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch
import torch.nn as nn

from .. import _lib
from .._lib import call, ptr, stream

_I = _lib.c_int


def _conv_bn_relu(cin: int, cout: int, k: int, bias: bool) -> nn.Sequential:
    return nn.Sequential(nn.Conv2d(cin, cout, k, padding=k // 2, bias=bias), nn.BatchNorm2d(cout), nn.ReLU(True))


def _reference_init(root: nn.Module) -> None:
    """Kaiming-normal(fan_out, relu) on every conv weight (biases keep their default
    init), BN gamma = beta = 0.1; reference model/tactileSR_model.py:92-98,208-214."""
    for m in root.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
        elif isinstance(m, nn.BatchNorm2d):
            nn.init.constant_(m.weight, 0.1)
            nn.init.constant_(m.bias, 0.1)


_HOLD = "_tsr_hold_bn_prev"      # on a marked nn.BatchNorm2d: the `training` flag it had when it was marked


def hold_bn_statistics(module: nn.Module, hold: bool = True) -> nn.Module:
    """Fine-tune on fixed statistics: put every ``nn.BatchNorm2d`` under `module` in eval mode and MARK it, so that the
    ``train()`` of ``TactileSR`` / ``MSRB`` / ``ResBlock`` (a trainer's per-epoch ``model.train()``) does not undo it.  The
    train step then normalises those layers with their running statistics, leaves ``running_mean`` / ``running_var`` /
    ``num_batches_tracked`` alone and runs the eval-mode backward (torch's ``bn.eval()`` inside a training module; a plain
    ``bn.eval()`` without the mark is honoured the same way until the next ``train()``).  ``hold=False`` clears the mark and
    restores the mode the layer had when it was marked.  No parameter, buffer or ``state_dict`` key changes."""
    for m in module.modules():
        if isinstance(m, nn.BatchNorm2d):
            if hold:
                if not hasattr(m, _HOLD):
                    setattr(m, _HOLD, m.training)
                m.training = False
            elif hasattr(m, _HOLD):
                m.training = getattr(m, _HOLD)
                delattr(m, _HOLD)
    return module


def _reapply_hold(root: nn.Module) -> None:
    for m in root.modules():
        if isinstance(m, nn.BatchNorm2d) and hasattr(m, _HOLD):
            m.training = False


class _PlanCache:
    """Repack when a parameter changed: `_get_plan()` is the class's `_build_plan()`, built again whenever one of its
    `_plan_fields` attributes, a parameter or a buffer (address or version), the `eps` of a BatchNorm layer (the fold bakes
    it into scale / shift), the library's parameter epoch or the module's own `_plan_gen` (`.half()` / `.float()` / `.to()`)
    has moved.

    The rule for writers: anything that bumps the tensor's version counter or replaces the tensor is seen -- in-place ops
    under ``no_grad``, ``load_state_dict``, ``torch.optim`` steps, ``module.half().float()``, ``reset_running_stats()`` --
    and the package's own writers (``optim.Adam``, ``WeightEMA``, ``recalibrate_bn``, the train step, ``GraphedTrainStep``)
    bump the epoch.  An in-place edit through ``.data`` (``p.data.mul_(2)``) moves neither address nor version and CANNOT
    be seen: follow it with ``tactilesr_amd.invalidate_weight_packs()``."""
    _plan_fields = ("conv_impl",)

    _plan_gen = 0        # moved by `_apply` (.half() / .float() / .to() of this module or of a parent)

    def _param_key(self):
        key = [getattr(self, f) for f in self._plan_fields]
        key.append(_lib.param_epoch())
        for m in self.modules():         # one walk of the tree: every parameter and buffer, every BatchNorm eps, every generation
            for t in m._parameters.values():
                if t is not None:
                    key.append(t.data_ptr())
                    key.append(t._version)
            for t in m._buffers.values():
                if t is not None:
                    key.append(t.data_ptr())
                    key.append(t._version)
            if isinstance(m, nn.BatchNorm2d):
                key.append(m.eps)
            else:
                key.append(m.__dict__.get("_plan_gen", 0))
        return tuple(key)

    def _apply(self, fn, *args, **kwargs):
        # .half() / .float() / .to(): `param.data = fn(param.data)` bumps no version, and the caching allocator may hand the
        # new tensor the address the old one just released
        out = super()._apply(fn, *args, **kwargs)
        self._plan_gen += 1
        return out

    def _get_plan(self):
        key = self._param_key()
        if self._plan is None or key != self._plan_key:
            self._plan, self._plan_key = self._build_plan(), key
        return self._plan


class _StandaloneBlock(_PlanCache, nn.Module):
    """Shared forward of the standalone ``MSRB`` / ``ResBlock`` modules (the whole-network engine of ``TactileSR`` runs
    the same kernels on its own buffers): ``block(x)`` with x ``(B, 64, H, W)`` fp32 NCHW on a ROCm device.  Eval mode
    runs the inference launches (fp16x3 by default: stage-1 pair kernel, fused 1x1) and returns a plain tensor; train
    mode runs batch-statistics BatchNorm through ``model/_train.py`` and is differentiable (x and parameters)."""
    _kind = ""
    _profile = None

    def _standalone_init(self):
        # arithmetic of the eval / train launches: attributes, set explicitly (no environment variable changes them)
        self.conv_impl = "fp16x3"
        self.train_impl = "fp16x3"
        self._plan = self._plan_key = self._block_engine = None

    def extra_repr(self):
        return f"arithmetic: eval conv_impl={self.conv_impl!r}, train_impl={self.train_impl!r}"

    def train(self, mode: bool = True):
        super().train(mode)
        _reapply_hold(self)          # hold_bn_statistics: marked BatchNorm layers stay in eval mode
        return self

    def block_engine(self):
        if self.train_impl not in ("fp16x3", "bf16x6", "f32"):
            # the bf16-storage step is only pinned for the whole network (against the bf16-emulating oracle)
            raise _lib.TactileSRHipError(f"standalone {type(self).__name__}: train_impl {self.train_impl!r} is not "
                                         "available (fp16x3, bf16x6, f32)")
        if self._block_engine is None or self._block_engine.impl != self.train_impl:
            from ._train import BlockEngine
            old = self._block_engine
            self._block_engine = BlockEngine(self, self._kind, self.train_impl)
            if old is not None:
                self._block_engine.keep_ctx, self._block_engine.grad_sync = old.keep_ctx, old.grad_sync
        return self._block_engine

    def forward(self, x):
        if not x.is_cuda:
            raise _lib.TactileSRHipError(f"{type(self).__name__} (tactilesr_amd) runs on MI355X only: move the module and "
                                         "its input to a ROCm device (no CPU fallback)")
        assert x.dim() == 4 and x.shape[1] == 64, "MSRB / ResBlock take (B, 64, H, W) feature maps"
        if self.conv_impl not in ("fp16x3", "bf16x6", "f32"):
            raise _lib.TactileSRHipError(f"standalone {type(self).__name__}: conv_impl {self.conv_impl!r} is not available "
                                         "(fp16x3, bf16x6, f32)")
        if self.training:
            from ._train import TrainFn
            named = list(self.named_parameters())
            xin = x.float().contiguous()
            return TrainFn.apply(self.block_engine(), [n for n, _ in named], xin, *[p for _, p in named])
        x = x.detach().float().contiguous()
        with torch.no_grad():
            return self._eval_forward(x)


class MSRB(_StandaloneBlock):
    """Multi-scale residual block (reference model/tactileSR_model.py:157-214):
    {3x3,5x5}@64 -> cat128 -> {3x3,5x5}@128 -> cat256 -> 1x1 -> +x -> ReLU."""
    _kind = "msrb"

    def __init__(self, n_feats: int = 64):
        super().__init__()
        self.conv_3_1 = _conv_bn_relu(n_feats, n_feats, 3, True)
        self.conv_5_1 = _conv_bn_relu(n_feats, n_feats, 5, True)
        self.conv_3_2 = _conv_bn_relu(2 * n_feats, 2 * n_feats, 3, True)
        self.conv_5_2 = _conv_bn_relu(2 * n_feats, 2 * n_feats, 5, True)
        self.confusion = nn.Conv2d(4 * n_feats, n_feats, 1, padding=0, stride=1)
        self.relu = nn.ReLU(inplace=True)
        _reference_init(self)
        self._standalone_init()

    def _build_plan(self):
        return _msrb_plan(self, CONV_IMPLS[self.conv_impl], True, True, False)

    def _eval_forward(self, x):
        B, _, H, W = x.shape
        slot = _SlotPool(4, x.device, CONV_IMPLS[self.conv_impl] == NS_F16X3)
        s_x, s_o = slot(), slot()
        if s_x is not None:
            s_x.copy_(x.abs().amax())
        xa = to_cb16(x)
        out = torch.empty_like(xa)
        plan = self._get_plan()
        ws = _msrb_workspace(plan.halves is not None, xa, B * H * W)
        _run_msrb(plan, self._profile, xa, s_x, out, 64, 0, s_o, ws, slot, B, H, W)
        return from_cb16(out, B, 64, H, W)


class ResBlock(_StandaloneBlock):
    """relu(x + conv2(relu(conv1(x)))) (reference model/tactileSR_model.py:216-225)."""
    _kind = "res"

    def __init__(self, n_feats: int = 64):
        super().__init__()
        self.conv1 = nn.Conv2d(n_feats, n_feats, kernel_size=3, padding=1)
        self.conv2 = nn.Conv2d(n_feats, n_feats, kernel_size=3, padding=1)
        self._standalone_init()

    def _build_plan(self):
        return _res_plan(self, CONV_IMPLS[self.conv_impl])

    def _eval_forward(self, x):
        B, _, H, W = x.shape
        slot = _SlotPool(3, x.device, CONV_IMPLS[self.conv_impl] == NS_F16X3)
        s_x, s_o = slot(), slot()
        if s_x is not None:
            s_x.copy_(x.abs().amax())
        xa = to_cb16(x)
        f1, out = torch.empty_like(xa), torch.empty_like(xa)
        _run_res(self._get_plan(), self._profile, xa, s_x, out, 64, 0, s_o, f1, slot, B, H, W)
        return from_cb16(out, B, 64, H, W)


# Arithmetic codes of the C ABI (`nsplit` of include/tactilesr_hip.h): 1..3 = that many bf16 planes, and
NS_F32 = 0          # fp32 MFMA
NS_F16X3 = -2       # two power-of-two-scaled fp16 planes, three products
NS_B16 = -1         # train: bf16 activation / gradient storage
NS_B16K = -3        # train: the bf16-storage forms that run on conv_b16k / conv1x1_b16k
NS_B16K_PAIR = -4   # train: the bf16-storage stage-1 pair (one 5x5 launch on conv_b16k)
CONV_IMPLS = {"f32": NS_F32, "bf16x6": 3, "bf16x3": 2, "bf16": 1, "fp16x3": NS_F16X3}   # eval: one plane = bf16 storage


def _pow2_wscale(max_abs: float) -> float:
    """fp16 planes: the power-of-two weight scale that puts max|w| * wscale in [2^13, 2^14)."""
    return 2.0 ** (13 - math.floor(math.log2(max_abs))) if max_abs > 0 else 1.0


class _SlotPool:
    """fp16x3: one device scalar per logical activation tensor holds max|x| (atomic max by the producer's epilogue; the
    consumer derives its power-of-two input scale from it).  `pool()` hands out the next 1-element view of ONE zeroed
    buffer; a pool that is not `enabled` (every other arithmetic) hands out None."""
    __slots__ = ("buf", "used")

    def __init__(self, n, device, enabled):
        self.buf = torch.zeros(n, dtype=torch.float32, device=device) if enabled else None
        self.used = 0

    def __call__(self):
        if self.buf is None:
            return None
        self.used += 1
        return self.buf[self.used - 1:self.used]


class _timed:
    """`with _timed(prof, key):` brackets the launches inside with two HIP events on the launch stream and appends the
    pair to `prof[key]` (bench.py); with `prof` None it does nothing and creates no event."""
    __slots__ = ("prof", "key", "ev")

    def __init__(self, prof, key):
        self.prof, self.key = prof, key

    def __enter__(self):
        if self.prof is not None:
            self.ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            self.ev[0].record()

    def __exit__(self, *exc):
        if self.prof is not None:
            self.ev[1].record()
            self.prof.setdefault(self.key, []).append(self.ev)
        return False


def _twin_args(io16, name, args, amax=()):
    """`call` arguments, but for the stream, of a glue launch that has an fp32 and a bf16-storage form: `name + "_b16"` under
    bf16 storage, else `name` -- which also takes the tensors in `amax` (the max|.| slot of what it writes) where the fp32
    form has that one more pointer."""
    return (name + "_b16", *args) if io16 else (name, *args, *map(ptr, amax))


def _pack_form(ns, out, cin, ks, dgrad=False, dev_amax=False):
    """The weight pack of arithmetic `ns` for a conv with `out` output and `cin` input channels (a data-gradient pack,
    `dgrad`: of the flipped conv, (out, cin) = (nprime, cout)): its entry point, the packed element count and dtype, and
    the arguments the entry point takes between the integers and the stream, but for the fp16 scale.  fp16 planes are
    scaled by a host float, or (`dev_amax`) from a device scalar max|w|."""
    name = "tsr_pack_conv_weight_dgrad" if dgrad else "tsr_pack_conv_weight"
    lib = _lib.load()
    if ns == NS_B16K:         # bf16 activation storage, the launch runs csrc/conv_b16k.hip: that kernel's slab layout
        return name + "_b16k", lib.tsr_conv_weight_b16k_elems(out, cin, ks), torch.bfloat16, ()
    if ns == NS_F16X3:
        return (name + ("_f16s_dev" if dev_amax else "_f16s"), lib.tsr_conv_weight_bf16s_elems(out, cin, ks, 2),
                torch.float16, ())
    if ns == NS_F32:
        return name, out * cin * ks * ks, torch.float32, ()
    ns = 1 if ns == NS_B16 else ns      # bf16 activation storage: the weights are the one-plane bf16 pack
    return name + "_bf16s", lib.tsr_conv_weight_bf16s_elems(out, cin, ks, ns), torch.bfloat16, (_I(ns),)


def _pack_pair_b16k(w3, w5):
    """bf16 storage: the weights of conv_3_1 || conv_5_1 as ONE 5x5 conv to 128 channels on conv_b16k (the 3x3 weight
    zero-padded into the inner taps of its half; the kernel skips the others)."""
    cin = w3.shape[1]
    w = torch.cat([torch.nn.functional.pad(w3, (1, 1, 1, 1)), w5], 0).contiguous()
    wp = torch.empty(_lib.load().tsr_conv_weight_b16k_pair_elems(cin), dtype=torch.bfloat16, device=w.device)
    call("tsr_pack_conv_weight_b16k_pair", ptr(w), ptr(wp), _I(cin), stream())
    return wp


def _pack_host(w, ns):
    """Pack the (cout, cin, ks, ks) weight `w` for an eval launch of arithmetic `ns`: (packed weight, w_inv_scale) -- fp16
    planes are scaled by the power of two the host derives from max|w|, everything else is not scaled."""
    cout, cin, ks = w.shape[0], w.shape[1], w.shape[2]
    name, n, dtype, tail = _pack_form(ns, cout, cin, ks)
    inv = 1.0
    if ns == NS_F16X3:
        wscale = _pow2_wscale(float(w.abs().max()))
        tail, inv = (_lib.c_float(wscale),), 1.0 / wscale
    wp = torch.empty(n, dtype=dtype, device=w.device)
    call(name, ptr(w), ptr(wp), _I(cout), _I(cin), _I(ks), *tail, stream())
    return wp, inv


class _PackedConv:
    """Device-side constants of one conv launch: packed weight, folded scale/shift."""
    __slots__ = ("w", "scale", "shift", "cin", "cout", "ks", "nsplit", "w_inv_scale", "io16", "b16k")

    def __init__(self, conv: nn.Conv2d, bn: Optional[nn.BatchNorm2d], nsplit: int = 0, cin_perm=None):
        w = conv.weight.detach().float()
        if cin_perm is not None:         # the producer wrote its channels in another order (stage-1 pair kernel)
            w = w[:, cin_perm]
        w = w.contiguous()
        self.cout, self.cin, self.ks = w.shape[0], w.shape[1], w.shape[2]
        self.nsplit = nsplit
        self.io16 = nsplit == CONV_IMPLS["bf16"]
        # bf16 activation storage (one plane is only ever that path's): the 3x3 / 5x5 convs run csrc/conv_b16k.hip
        # (its 64-channel instantiations -- 16 MFMAs per barrier step -- measure slower than the 32x32x16 kernel's 3-tap steps:
        #  3x3 64->64 0.83 vs 0.70 ms per launch at B = 4096; they stay on that kernel)
        self.b16k = self.io16 and self.ks > 1 and self.cin % 32 == 0 and self.cout == 128
        self.w, self.w_inv_scale = _pack_host(w, NS_B16K if self.b16k else nsplit)
        self.scale, self.shift = _fold(conv.bias, bn, self.cout, w.device)


class _PackedPair:
    """Stage-1 pair of an MSRB (conv_3_1 || conv_5_1 on the same input) as one launch of the K = 32 kernel: packed weight
    stream, folded BN scale / shift in the kernel's channel order, and that order (`perm[k]` = channel of
    cat([conv3, conv5]) held by kernel channel k) for the consumers' weights."""
    __slots__ = ("w", "scale", "shift", "cin", "w_inv_scale", "perm")
    b16k = False
    _perm = None

    @classmethod
    def channel_perm(cls, device):
        if cls._perm is None:
            import ctypes
            arr = (ctypes.c_int * 128)()
            call("tsr_pair_channel_perm", ctypes.cast(arr, ctypes.c_void_p))
            cls._perm = list(arr)
        return torch.tensor(cls._perm, dtype=torch.long, device=device)

    def __init__(self, seq3: nn.Sequential, seq5: nn.Sequential):
        w3 = seq3[0].weight.detach().float().contiguous()
        w5 = seq5[0].weight.detach().float().contiguous()
        self.cin = w3.shape[1]
        wscale = _pow2_wscale(max(float(w3.abs().max()), float(w5.abs().max())))
        self.w_inv_scale = 1.0 / wscale
        self.w = torch.empty(_lib.load().tsr_conv_weight_pair_elems(self.cin), dtype=torch.float16, device=w3.device)
        call("tsr_pack_conv_weight_pair_f16s", ptr(w3), ptr(w5), ptr(self.w), _I(self.cin), _lib.c_float(wscale),
             ptr(None), stream())
        s3, sh3 = _fold(seq3[0].bias, seq3[1], 64, w3.device)
        s5, sh5 = _fold(seq5[0].bias, seq5[1], 64, w3.device)
        self.perm = self.channel_perm(w3.device)
        self.scale = torch.cat([s3, s5])[self.perm].contiguous()
        self.shift = torch.cat([sh3, sh5])[self.perm].contiguous()


class _PackedPairB16:
    """Stage-1 pair of an MSRB for the bf16-storage path: ONE 5x5 conv to 128 channels whose first 64 output channels are
    conv_3_1 (its 3x3 weight zero-padded to 5x5; the kernel skips those taps) and whose last 64 are conv_5_1 -- packed by
    the ordinary one-plane pack -- with the two folded BatchNorm vectors concatenated.  `cat1` comes out in torch.cat order."""
    __slots__ = ("w", "scale", "shift", "cin")
    b16k = True
    perm = None          # `cat1` in torch.cat order: nothing to permute downstream

    def __init__(self, seq3: nn.Sequential, seq5: nn.Sequential):
        w3 = seq3[0].weight.detach().float()
        w5 = seq5[0].weight.detach().float()
        self.cin = w3.shape[1]
        self.w = _pack_pair_b16k(w3, w5)
        s3, sh3 = _fold(seq3[0].bias, seq3[1], 64, w3.device)
        s5, sh5 = _fold(seq5[0].bias, seq5[1], 64, w3.device)
        self.scale = torch.cat([s3, s5]).contiguous()
        self.shift = torch.cat([sh3, sh5]).contiguous()


class _PackedHalf:
    """One 64x128x1x1 half of an MSRB's `confusion` weight in the fp16 two-plane pack (fused 1x1 epilogue)."""
    __slots__ = ("w", "w_inv_scale")

    def __init__(self, w: torch.Tensor, ns: int):
        w = w.float().contiguous()
        if ns != NS_F16X3:        # bf16-storage path: one bf16 plane, no scaling
            self.w_inv_scale = 1.0
            self.w = torch.empty(64 * 128, dtype=torch.bfloat16, device=w.device)
            call("tsr_pack_w2_b16k", ptr(w), ptr(self.w), stream())
            return
        self.w, self.w_inv_scale = _pack_host(w, NS_F16X3)


def _fold(bias, bn: Optional[nn.BatchNorm2d], cout: int, device):
    """Eval-mode BatchNorm2d folded onto the conv output: y = conv*scale + shift with
    scale = gamma/sqrt(var+eps), shift = (bias-mean)*scale + beta."""
    if bn is None:
        if bias is None:
            return None, None
        return None, bias.detach().float().contiguous()
    scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
    b = bias.detach().float() if bias is not None else torch.zeros(cout, device=device)
    shift = (b - bn.running_mean.detach().float()) * scale + bn.bias.detach().float()
    return scale.contiguous(), shift.contiguous()


class _MSRBPlan:
    """Packed constants of one MSRB.  Stage 1 is either `pair` (one launch; `c31` / `c51` None) or the two convs `c31` /
    `c51` (`pair` None); `halves` = the two 64x128 halves of the 1x1 `confusion` for the fused stage 2, or None (stage 2
    writes `cat2` and `conf` runs as a launch of its own; fused, only `conf.shift` is read)."""
    __slots__ = ("pair", "c31", "c51", "c32", "c52", "conf", "halves")


class _ResPlan:
    __slots__ = ("c1", "c2")


def _msrb_plan(blk, ns, fuse_pair, fuse_1x1, bf16_storage) -> _MSRBPlan:
    """Pack one MSRB for arithmetic `ns`.  `fuse_pair` / `fuse_1x1` take effect where the kernels exist: fp16x3 and the
    bf16-storage path."""
    p = _MSRBPlan()
    has_fused = ns == NS_F16X3 or bf16_storage
    p.halves = p.pair = p.c31 = p.c51 = None
    if fuse_1x1 and has_fused:
        p.halves = tuple(_PackedHalf(blk.confusion.weight.detach()[:, o:o + 128], ns) for o in (0, 128))
    if fuse_pair and has_fused:
        # stage 1 as ONE launch (3x3 || 5x5 on one staged halo); the fp16x3 kernel leaves cat1 in its own channel order
        # and the stage-2 weights are permuted along C_in to match
        p.pair = (_PackedPairB16 if bf16_storage else _PackedPair)(blk.conv_3_1, blk.conv_5_1)
    else:
        p.c31 = _PackedConv(blk.conv_3_1[0], blk.conv_3_1[1], ns)
        p.c51 = _PackedConv(blk.conv_5_1[0], blk.conv_5_1[1], ns)
    perm = p.pair.perm if p.pair is not None else None
    p.c32 = _PackedConv(blk.conv_3_2[0], blk.conv_3_2[1], ns, cin_perm=perm)
    p.c52 = _PackedConv(blk.conv_5_2[0], blk.conv_5_2[1], ns, cin_perm=perm)
    p.conf = _PackedConv(blk.confusion, None, ns)
    return p


def _res_plan(rb, ns) -> _ResPlan:
    p = _ResPlan()
    p.c1, p.c2 = _PackedConv(rb.conv1, None, ns), _PackedConv(rb.conv2, None, ns)
    return p


def _conv(prof, pc: _PackedConv, src, s_ctot, s_coff, dst, d_ctot, d_coff, relu, B, H, W, res=None, r_ctot=0, r_coff=0,
          amax_in=None, amax_out=None):
    with _timed(prof, (pc.ks, pc.cout)):     # bench.py: per kernel instantiation
        if pc.io16:      # bf16 activation storage
            call("tsr_conv2d_fwd_b16k" if pc.b16k else "tsr_conv2d_fwd_b16", ptr(src), _I(s_ctot), _I(s_coff), _I(pc.cin),
                 ptr(pc.w), _I(pc.cout), _I(pc.ks), ptr(pc.scale), ptr(pc.shift), ptr(res), _I(r_ctot), _I(r_coff),
                 ptr(dst), _I(d_ctot), _I(d_coff), _I(1 if relu else 0), _I(B), _I(H), _I(W), stream())
        elif pc.nsplit == NS_F16X3:
            call("tsr_conv2d_fwd_f16s", ptr(src), _I(s_ctot), _I(s_coff), _I(pc.cin), ptr(pc.w), _I(pc.cout),
                 _I(pc.ks), _lib.c_float(pc.w_inv_scale), ptr(amax_in), ptr(amax_out), ptr(pc.scale), ptr(pc.shift),
                 ptr(res), _I(r_ctot), _I(r_coff), ptr(dst), _I(d_ctot), _I(d_coff), _I(1 if relu else 0),
                 _I(B), _I(H), _I(W), stream())
        elif pc.nsplit == NS_F32:
            call("tsr_conv2d_fwd", ptr(src), _I(s_ctot), _I(s_coff), _I(pc.cin), ptr(pc.w), _I(pc.cout), _I(pc.ks),
                 ptr(pc.scale), ptr(pc.shift), ptr(res), _I(r_ctot), _I(r_coff),
                 ptr(dst), _I(d_ctot), _I(d_coff), _I(1 if relu else 0), _I(B), _I(H), _I(W), stream())
        else:
            call("tsr_conv2d_fwd_bf16s", ptr(src), _I(s_ctot), _I(s_coff), _I(pc.cin), ptr(pc.w), _I(pc.cout),
                 _I(pc.ks), _I(pc.nsplit), ptr(pc.scale), ptr(pc.shift), ptr(res), _I(r_ctot), _I(r_coff),
                 ptr(dst), _I(d_ctot), _I(d_coff), _I(1 if relu else 0), _I(B), _I(H), _I(W), stream())


def _conv_pair(prof, pp, src, dst, B, H, W, amax_in, amax_out):
    """conv_3_1 || conv_5_1 (+ BN + ReLU each) of an MSRB: 64 -> 128 channels of `cat1`, one launch."""
    with _timed(prof, ("pair", 128)):
        if pp.b16k:
            call("tsr_conv2d_fwd_b16k_pair", ptr(src), _I(64), _I(0), _I(pp.cin), ptr(pp.w), ptr(pp.scale), ptr(pp.shift),
                 ptr(dst), _I(128), _I(0), _I(1), _I(B), _I(H), _I(W), stream())
        else:
            call("tsr_conv2d_fwd_f16s_pair", ptr(src), _I(64), _I(0), _I(pp.cin), ptr(pp.w), _lib.c_float(pp.w_inv_scale),
                 ptr(amax_in), ptr(amax_out), ptr(pp.scale), ptr(pp.shift), ptr(dst), _I(128), _I(0), _I(1),
                 _I(B), _I(H), _I(W), stream())


def _conv_fused(prof, pc: _PackedConv, half: _PackedHalf, shift2, src, dst, d_ctot, d_coff, res, r_ctot, r_coff, relu2,
                amax_out, amax_in, B, H, W):
    """Stage-2 conv (128 -> 128, BN + ReLU) + its half of the 1x1 confusion + residual (+ ReLU), one launch."""
    with _timed(prof, (pc.ks, pc.cout)):
        if pc.io16:
            call("tsr_conv2d_fwd_b16k_fuse1x1", ptr(src), _I(128), _I(0), _I(128), ptr(pc.w), _I(pc.ks), ptr(pc.scale),
                 ptr(pc.shift), _I(1), ptr(half.w), ptr(shift2), ptr(res), _I(r_ctot), _I(r_coff), ptr(dst), _I(d_ctot),
                 _I(d_coff), _I(1 if relu2 else 0), _I(B), _I(H), _I(W), stream())
        else:
            call("tsr_conv2d_fwd_f16s_fuse1x1", ptr(src), _I(128), _I(0), _I(128), ptr(pc.w), _I(pc.ks),
                 _lib.c_float(pc.w_inv_scale), ptr(amax_in), ptr(amax_out), ptr(pc.scale), ptr(pc.shift), _I(1),
                 ptr(half.w), _lib.c_float(half.w_inv_scale), ptr(shift2), ptr(res), _I(r_ctot), _I(r_coff),
                 ptr(dst), _I(d_ctot), _I(d_coff), _I(1 if relu2 else 0), _I(B), _I(H), _I(W), stream())


def _msrb_workspace(fused: bool, like: torch.Tensor, BHW: int):
    """Scratch of `_run_msrb`, reusable from block to block: `cat1` (128 channels) and, with the 1x1 fused, the partial
    sum `p1` (64) -- else `cat2` (256)."""
    return like.new_empty(128 * BHW), like.new_empty((64 if fused else 256) * BHW)


def _run_msrb(p: _MSRBPlan, prof, src, s_in, dst, d_ctot, d_coff, s_out, ws, slot, B, H, W):
    """The eval launches of one MSRB: the 64-channel CB16 buffer `src` -> channels [d_coff, d_coff + 64) of `dst`.
    `s_in` / `s_out`: the max|.| slots of the input / output tensor, `slot`: the pool the block's own two come from."""
    cat1, ws2 = ws
    s_c1, s_c2 = slot(), slot()
    if p.pair is not None:
        _conv_pair(prof, p.pair, src, cat1, B, H, W, s_in, s_c1)
    else:
        _conv(prof, p.c31, src, 64, 0, cat1, 128, 0, True, B, H, W, amax_in=s_in, amax_out=s_c1)
        _conv(prof, p.c51, src, 64, 0, cat1, 128, 64, True, B, H, W, amax_in=s_in, amax_out=s_c1)
    if p.halves is not None:
        # stage 2 with the 1x1 fused: P = W_a.relu(bn(conv3)) + b + x ; out = relu(W_b.relu(bn(conv5)) + P)
        _conv_fused(prof, p.c32, p.halves[0], p.conf.shift, cat1, ws2, 64, 0, src, 64, 0, False, None, s_c1, B, H, W)
        _conv_fused(prof, p.c52, p.halves[1], None, cat1, dst, d_ctot, d_coff, ws2, 64, 0, True, s_out, s_c1, B, H, W)
    else:
        _conv(prof, p.c32, cat1, 128, 0, ws2, 256, 0, True, B, H, W, amax_in=s_c1, amax_out=s_c2)
        _conv(prof, p.c52, cat1, 128, 0, ws2, 256, 128, True, B, H, W, amax_in=s_c1, amax_out=s_c2)
        _conv(prof, p.conf, ws2, 256, 0, dst, d_ctot, d_coff, True, B, H, W, res=src, r_ctot=64, r_coff=0,
              amax_in=s_c2, amax_out=s_out)


def _run_res(p: _ResPlan, prof, src, s_in, dst, d_ctot, d_coff, s_out, f1, slot, B, H, W):
    """The eval launches of one ResBlock: `src` (64 channels) -> channels [d_coff, d_coff + 64) of `dst`; `f1`: scratch."""
    s_1 = slot()
    _conv(prof, p.c1, src, 64, 0, f1, 64, 0, True, B, H, W, amax_in=s_in, amax_out=s_1)
    _conv(prof, p.c2, f1, 64, 0, dst, d_ctot, d_coff, True, B, H, W, res=src, r_ctot=64, r_coff=0, amax_in=s_1,
          amax_out=s_out)


class TactileSR(_PlanCache, nn.Module):
    """STSR / MTSR taxel super-resolution network on MI355X.

    ``model(LR)`` with LR ``(B, seqsCnt*axisCnt, 4, 4)`` fp32 on a ROCm device returns
    ``(B, 1, 4*scale_factor, 4*scale_factor)``, numerically equal (<=1e-5 relative) to
    the reference forward (model/tactileSR_model.py:67-84).  Any other taxel grid and ``axisCnt != 3`` are refused
    before the first launch: the reference resizes its output to ``(4*scale_factor, 4*scale_factor)`` whatever the
    grid, and the stem kernels are 3-axis.  ``seqsCnt`` and the two block counts are free (a count of 0 copies that
    branch's input into the head's input; the train step and the bf16-storage path need both counts >= 1).
    """
    _plan_fields = ("conv_impl", "head_impl", "fuse_1x1", "fuse_pair")

    def __init__(self, scale_factor=10, seqsCnt=1, axisCnt=3, patternFeatureExtraLayerCnt=6,
                 forceFeatureExtraLayerCnt=1, *, conv_impl: str = "fp16x3", train_impl: str = "fp16x3"):
        super().__init__()
        self.taxel_cnt = 4
        self.scale_factor = scale_factor
        self.seqsCnt = seqsCnt
        self.axisCnt = axisCnt

        # construction order == RNG order of the reference (blocks first, then stems)
        self.patternFeatureExtra_layer = self.make_layer(MSRB, patternFeatureExtraLayerCnt)
        self.forceFeatureExtra_layer = self.make_layer(ResBlock, forceFeatureExtraLayerCnt)
        self.inputLayer_pattern_list = nn.ModuleList()
        for _ in range(seqsCnt):
            self.inputLayer_pattern_list.append(nn.Sequential(
                nn.Upsample(scale_factor=scale_factor, mode="bilinear", align_corners=False),
                nn.Conv2d(axisCnt, 64, 3, padding=1, bias=False), nn.BatchNorm2d(64), nn.ReLU(True),
                nn.Conv2d(64, 64, 3, padding=1, bias=False), nn.BatchNorm2d(64), nn.ReLU(True)))
        self.inputContact_layer = nn.Sequential(
            nn.Conv2d(seqsCnt * 64, 64, 3, padding=1, bias=False), nn.BatchNorm2d(64), nn.ReLU(True))
        self.output_layer = nn.Sequential(
            nn.Conv2d(128, 128, 3, padding=1, bias=False), nn.ReLU(True),
            nn.Conv2d(128, 1, 3, padding=1, bias=False), nn.ReLU(True))
        self.input_layer_force = nn.Sequential(
            nn.Upsample(scale_factor=scale_factor, mode="bilinear", align_corners=False),
            nn.Conv2d(axisCnt, 64, 3, padding=1, bias=False), nn.ReLU(True))
        self._init_network()
        self._plan = None
        self._plan_key = None
        self._profile = None
        self._train_engine = None
        # eval-mode conv arithmetic (all accumulate in fp32):
        #   "fp16x3" (default) 2 power-of-two-scaled fp16 planes, 3 f16-MFMA products: fp32-grade at 3/16 the fp32-MFMA cost
        #   "bf16x6"           3 bf16 planes, 6 bf16-MFMA products: fp32-equivalent, no scaling needed
        #   "f32"              fp32 MFMA (exact fp32 fma chain)
        #   "bf16x3"           reduced precision (never the parity path)
        #   "bf16"             BASELINE's "bf16" configurations: bf16 ACTIVATION STORAGE in HBM + plain bf16 MFMA operands,
        #                      fp32 accumulate (tolerance 2e-2; never the parity path)
        # The arithmetic is chosen EXPLICITLY -- the two keyword-only constructor arguments above or these attributes --
        # and printed by repr(model); no environment variable changes it (a stray TSR_* variable on a user's box must not
        # silently change precision).  The defaults are the parity paths.
        if conv_impl not in CONV_IMPLS:
            raise _lib.TactileSRHipError(f"conv_impl {conv_impl!r}: expected one of {sorted(CONV_IMPLS)}")
        self.conv_impl = conv_impl
        # train-step arithmetic (model/_train.py): "fp16x3" (default, fp32-grade), "bf16x6", "f32", "bf16" = bf16 activation /
        # gradient STORAGE + bf16 MFMA operands (BASELINE's "bf16" configurations; reduced precision), "bf16op"
        self.train_impl = train_impl
        # arithmetic of output_layer.0 (the 128->128 conv in front of the cancellation-heavy 128->1 head); None = conv_impl
        self.head_impl = None
        # fp16x3 eval: apply each half of an MSRB's 1x1 `confusion` inside the stage-2 conv that produced its input
        # (csrc/conv_fuse1x1.h): `cat2` never exists in HBM.  False keeps the separate 1x1 launches (same arithmetic).
        self.fuse_1x1 = True
        # eval, fp16x3: the two stage-1 convs of an MSRB as one launch on one staged halo (False: two launches)
        self.fuse_pair = True
        self.max_images_per_pass = 4096   # workspace bound: ~6.6 MB of CB16 activations per image

    def make_layer(self, block, num_of_layer):
        return nn.Sequential(*[block() for _ in range(num_of_layer)])

    def _init_network(self):
        _reference_init(self)

    def train(self, mode: bool = True):
        super().train(mode)
        _reapply_hold(self)          # hold_bn_statistics: marked BatchNorm layers stay in eval mode
        return self

    # ------------------------------------------------------------------ engine
    def _build_plan(self):
        """Pack weights / fold eval-mode BN once per parameter version."""
        plan: Dict[str, object] = {}
        ns = CONV_IMPLS[self.conv_impl]
        if self.head_impl is not None and self.head_impl not in CONV_IMPLS:
            raise _lib.TactileSRHipError(f"head_impl {self.head_impl!r}: expected one of {sorted(CONV_IMPLS)}")
        if self.conv_impl == "bf16" and self.head_impl not in (None, "bf16"):
            # the bf16-storage path hands bf16 CB16 buffers (half the bytes) to every kernel: an fp32-activation kernel
            # for output_layer.0 would read past them
            raise _lib.TactileSRHipError("head_impl cannot be combined with conv_impl='bf16' (bf16 activation storage): "
                                         "every launch of that path reads and writes bf16 tensors")
        if self.conv_impl != "bf16" and self.head_impl == "bf16":
            raise _lib.TactileSRHipError("head_impl='bf16' needs conv_impl='bf16' (it reads bf16 activation tensors)")
        stems = []
        for seq in self.inputLayer_pattern_list:
            s1, sh1 = _fold(None, seq[2], 64, seq[1].weight.device)
            stems.append((seq[1].weight.detach().float().contiguous(), s1, sh1, _PackedConv(seq[4], seq[5], ns)))
        plan["stems"] = stems
        plan["fuse"] = _PackedConv(self.inputContact_layer[0], self.inputContact_layer[1], ns)
        plan["msrb"] = [_msrb_plan(blk, ns, self.fuse_pair, self.fuse_1x1, self.conv_impl == "bf16")
                        for blk in self.patternFeatureExtra_layer]
        plan["force_w"] = self.input_layer_force[1].weight.detach().float().contiguous()
        plan["res"] = [_res_plan(rb, ns) for rb in self.forceFeatureExtra_layer]
        plan["head0"] = _PackedConv(self.output_layer[0], None, CONV_IMPLS[self.head_impl] if self.head_impl else ns)
        plan["head_w"] = self.output_layer[2].weight.detach().float().contiguous()
        return plan

    def _infer_pass(self, x: torch.Tensor, out: torch.Tensor, stages=None) -> None:
        """Eval-mode forward of one batch slice; mirrors reference forward :67-84."""
        plan = self._get_plan()
        B, hin, win = x.shape[0], x.shape[2], x.shape[3]
        sf, T, A = self.scale_factor, self.seqsCnt, self.axisCnt
        H, W = hin * sf, win * sf
        HW = H * W
        dev = x.device

        io16 = self.conv_impl == "bf16"       # activations stored as bf16 CB16 between the kernels
        if io16 and (len(plan["msrb"]) == 0 or len(plan["res"]) == 0):
            raise _lib.TactileSRHipError("the bf16-storage path needs at least one MSRB and one ResBlock")

        def buf(c):
            return torch.empty(B * c * HW, dtype=torch.bfloat16 if io16 else torch.float32, device=dev)

        def stem(coff, w1, s1, sh1, dst, slot_):
            call(*_twin_args(io16, "tsr_stem_fwd", (ptr(x), _I(ctot), _I(coff), _I(A), _I(hin), _I(win), _I(sf), ptr(w1),
                                                    ptr(s1), ptr(sh1), ptr(dst), _I(64), _I(0), _I(1), _I(B)), (slot_,)),
                 stream())

        ctot = x.shape[1]
        prof = self._profile
        slot = _SlotPool(16 + 8 * len(plan["msrb"]) + 4 * len(plan["res"]) + T, dev,
                         CONV_IMPLS[self.conv_impl] == NS_F16X3)
        stemA, catT = buf(64), buf(64 * T)
        s_catT = slot()
        for t, (w1, s1, sh1, pc2) in enumerate(plan["stems"]):
            s_stem = slot()
            stem(A * t, w1, s1, sh1, stemA, s_stem)
            _conv(prof, pc2, stemA, 64, 0, catT, 64 * T, 64 * t, True, B, H, W, amax_in=s_stem, amax_out=s_catT)
        xa, xb = buf(64), buf(64)
        s_x = slot()
        _conv(prof, plan["fuse"], catT, 64 * T, 0, xa, 64, 0, True, B, H, W, amax_in=s_catT, amax_out=s_x)
        if stages is not None:
            stages["stems"] = (catT, 64 * T)
            stages["fuse"] = (xa.clone(), 64)
        del stemA
        hcat = buf(128)
        s_hcat = slot()
        n_msrb = len(plan["msrb"])
        ws = _msrb_workspace(n_msrb > 0 and plan["msrb"][0].halves is not None, xa, B * HW)
        if n_msrb == 0:
            call("tsr_cb16_to_nchw", ptr(xa), ptr(xb), _I(B), _I(64), _I(HW), _I(64), _I(0), stream())
            call("tsr_nchw_to_cb16", ptr(xb), ptr(hcat), _I(B), _I(64), _I(HW), _I(128), _I(64), stream())
            if s_hcat is not None:    # the copy has no epilogue to raise the slot: hcat's bound must cover the copied half
                torch.maximum(s_hcat, s_x, out=s_hcat)
        cur, nxt = xa, xb
        for i, p in enumerate(plan["msrb"]):
            if i == n_msrb - 1:   # pattern feature lands in channels [64,128) of the head input (cat: force first)
                dst, s_out = (hcat, 128, 64), s_hcat
            else:
                dst, s_out = (nxt, 64, 0), slot()
            _run_msrb(p, prof, cur, s_x, *dst, s_out, ws, slot, B, H, W)
            if stages is not None:
                stages[f"msrb{i}"] = (dst[0].clone(),) + dst[1:]
            cur, nxt, s_x = nxt, cur, s_out
        del ws
        # force branch
        f0, f1 = buf(64), buf(64)
        s_f = slot()
        stem(0, plan["force_w"], None, None, f0, s_f)
        if stages is not None:
            stages["force_in"] = (f0.clone(), 64, 0)
        n_res = len(plan["res"])
        if n_res == 0:
            call("tsr_cb16_to_nchw", ptr(f0), ptr(f1), _I(B), _I(64), _I(HW), _I(64), _I(0), stream())
            call("tsr_nchw_to_cb16", ptr(f1), ptr(hcat), _I(B), _I(64), _I(HW), _I(128), _I(0), stream())
            if s_hcat is not None:
                torch.maximum(s_hcat, s_f, out=s_hcat)
        cur, nxt = f0, (buf(64) if n_res > 1 else None)
        for i, p in enumerate(plan["res"]):
            if i == n_res - 1:
                dst, s_out = (hcat, 128, 0), s_hcat
            else:
                dst, s_out = (nxt, 64, 0), slot()
            _run_res(p, prof, cur, s_f, *dst, s_out, f1, slot, B, H, W)
            if stages is not None and i < n_res - 1:      # (the last block's output is the stage "force")
                stages[f"res{i}"] = (dst[0].clone(),) + dst[1:]
            cur, nxt, s_f = nxt, cur, s_out
        h0 = buf(128)
        _conv(prof, plan["head0"], hcat, 128, 0, h0, 128, 0, True, B, H, W, amax_in=s_hcat, amax_out=None)
        if stages is not None:
            stages["force"] = (hcat, 128, 0)
            stages["head0"] = (h0, 128, 0)
        call(*_twin_args(io16, "tsr_head_fwd", (ptr(h0), _I(128), _I(128), ptr(plan["head_w"]), ptr(out), _I(1), _I(B), _I(H),
                                                _I(W))), stream())

    def _check_input(self, x):
        """What every forward (eval, train, `forward_with_stages`) refuses before its first launch: anything the
        reference's forward does not compute as this engine would."""
        assert x.shape[1] == self.seqsCnt * self.axisCnt, "input channel should be same with seqsCnt x axisCnt!"
        if self.axisCnt != 3:
            raise _lib.TactileSRHipError(f"TactileSR: axisCnt = {self.axisCnt} is not available: the stem kernels (pattern "
                                         "and force stems, their weight and taxel gradients) are written for 3-axis taxels")
        n = self.taxel_cnt
        if x.dim() != 4 or tuple(x.shape[2:]) != (n, n):
            raise _lib.TactileSRHipError(
                f"TactileSR: taxel grid {tuple(x.shape[2:])} is not available, only {n} x {n}: the reference ends with a "
                f"fixed output resize to ({n}*scale_factor, {n}*scale_factor) (model/tactileSR_model.py:83), an identity "
                f"on {n} x {n} taxels only; this engine has no such resize and would return another image")

    def forward(self, x):
        self._check_input(x)
        if not x.is_cuda:
            raise _lib.TactileSRHipError("TactileSR (tactilesr_amd) runs on MI355X only: move the model and "
                                         "its input to a ROCm device (no CPU fallback)")
        if self.training:
            # batch-statistics BatchNorm + autograd through the HIP backward (model/_train.py)
            from ._train import TrainFn
            named = list(self.named_parameters())
            # (not detached: with LR.requires_grad_() autograd routes d loss / d taxels back through .float() / slicing)
            out = TrainFn.apply(self.train_engine(), [n for n, _ in named], x.float().contiguous(), *[p for _, p in named])
            self._plan = None      # running statistics were updated in place by the kernels
            return out
        x = x.detach().float().contiguous()
        B = x.shape[0]
        H, W = x.shape[2] * self.scale_factor, x.shape[3] * self.scale_factor
        out = torch.empty(B, 1, H, W, dtype=torch.float32, device=x.device)
        step = max(2, int(self.max_images_per_pass))
        for b0 in range(0, B, step):
            b1 = min(B, b0 + step)
            self._infer_pass(x[b0:b1], out[b0:b1])
        return out

    def train_engine(self):
        """The module's HIP training engine for the current ``train_impl`` (created on first use; a changed
        ``train_impl`` gets a fresh engine that inherits the gradient arena / GradSync wiring -- a forward already
        recorded by autograd keeps the engine it ran on)."""
        eng = self._train_engine
        if eng is None or eng.impl != self.train_impl:
            from ._train import TrainEngine
            new = TrainEngine(self, self.train_impl)
            if eng is not None:
                new.keep_ctx, new.profile, new.n_buckets = eng.keep_ctx, eng.profile, eng.n_buckets
                new.arena, new.grad_sync = eng.arena, eng.grad_sync
            self._train_engine = new
        return self._train_engine

    def extra_repr(self):
        """First line of repr(model): the ACTIVE arithmetic of both modes."""
        grade = {"fp16x3": "fp32-grade: 2 scaled fp16 planes x 3 MFMA products", "bf16x6": "fp32-equivalent: 3 bf16 planes x 6",
                 "f32": "strict fp32 MFMA", "bf16": "REDUCED precision: bf16 storage + operands", "bf16x3": "REDUCED precision",
                 "bf16op": "REDUCED precision: bf16 operands"}
        head = f", head_impl={self.head_impl!r}" if self.head_impl else ""
        return (f"arithmetic: eval conv_impl={self.conv_impl!r} ({grade.get(self.conv_impl, '?')}){head}, "
                f"train_impl={self.train_impl!r} ({grade.get(self.train_impl, '?')}); fp32 accumulate everywhere")

    @torch.no_grad()
    def forward_with_stages(self, x):
        """Eval forward that also returns named intermediate activations converted to
        NCHW (parity probes against the oracle's ``stages``)."""
        assert not self.training
        self._check_input(x)
        x = x.detach().float().contiguous()
        B = x.shape[0]
        H, W = x.shape[2] * self.scale_factor, x.shape[3] * self.scale_factor
        out = torch.empty(B, 1, H, W, dtype=torch.float32, device=x.device)
        raw = {}
        self._infer_pass(x, out, raw)
        stages = {}
        for name, spec in raw.items():
            if name == "stems":
                t, ctot = spec
                for i in range(self.seqsCnt):
                    stages[f"stem{i}"] = _to_nchw(t, B, 64, H * W, ctot, 64 * i).view(B, 64, H, W)
                continue
            t, ctot = spec[0], spec[1]
            coff = spec[2] if len(spec) > 2 else 0
            c = 64 if name != "head0" else 128
            stages[name] = _to_nchw(t, B, c, H * W, ctot, coff).view(B, c, H, W)
        return out, stages


class TactileSRCNN(_PlanCache, nn.Module):
    """``TactileSRCNN`` of the reference (model/tactileSR_model.py:101-153): bilinear x10 -> three conv3x3+BN+ReLU
    (3->64, 64->64, 64->64) -> six MSRBs -> conv 64->1 + ReLU.  Both reference trainers import the name
    (train/tactileSR_train.py:24, train/tactileSRSeqs_train.py:24) and none instantiates it; it is exported so that
    import line works verbatim.  Same constructor (no arguments), submodule names, ``state_dict`` keys and seeded init.
    EVAL forward only, composed from the hot path's kernels (stem kernel, K = 32 conv, the MSRB launches, head kernel);
    train mode raises: the class is not on the path the trainers run."""

    def __init__(self):
        super().__init__()
        self.msrb_layer = nn.Sequential(*[MSRB() for _ in range(6)])
        self.input_zyx = nn.Sequential(
            nn.Conv2d(3, 64, 3, stride=1, padding=1, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True),
            nn.Conv2d(64, 64, 3, stride=1, padding=1, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True),
            nn.Conv2d(64, 64, 3, stride=1, padding=1, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True))
        self.upSample = nn.Upsample(scale_factor=10, mode="bilinear", align_corners=False)
        self.output = nn.Sequential(nn.Conv2d(64, 1, 3, stride=1, padding=1, bias=False), nn.ReLU(inplace=True))
        _reference_init(self)
        self.conv_impl = "fp16x3"            # explicit attribute, like TactileSR's (fp16x3 | bf16x6 | f32)
        self._profile = None
        self._plan = self._plan_key = None

    def extra_repr(self):
        return f"arithmetic: eval conv_impl={self.conv_impl!r} (train mode not available)"

    def _build_plan(self):
        ns = CONV_IMPLS[self.conv_impl]
        z = self.input_zyx
        s1, sh1 = _fold(None, z[1], 64, z[0].weight.device)
        return (z[0].weight.detach().float().contiguous(), s1, sh1, _PackedConv(z[3], z[4], ns),
                _PackedConv(z[6], z[7], ns), [_msrb_plan(blk, ns, True, True, False) for blk in self.msrb_layer],
                self.output[0].weight.detach().float().contiguous())

    def forward(self, x):
        if not x.is_cuda:
            raise _lib.TactileSRHipError("TactileSRCNN (tactilesr_amd) runs on MI355X only (no CPU fallback)")
        if self.training:
            raise _lib.TactileSRHipError(
                "TactileSRCNN: train mode is not on the MI355X path -- the reference's trainers import this class "
                "(train/tactileSR_train.py:24) but never instantiate it; only the eval forward is provided "
                "(call .eval()), TactileSR is the trainable model")
        if self.conv_impl not in ("fp16x3", "bf16x6", "f32"):
            raise _lib.TactileSRHipError(f"TactileSRCNN: conv_impl {self.conv_impl!r} is not available (fp16x3, bf16x6, f32)")
        assert x.dim() == 4 and x.shape[1] == 3, "TactileSRCNN takes (B, 3, h, w) taxel frames"
        x = x.detach().float().contiguous()
        with torch.no_grad():
            w1, s1, sh1, pc2, pc3, msrbs, wh = self._get_plan()
            B, _, hin, win = x.shape
            H, W = hin * 10, win * 10
            dev, prof = x.device, self._profile
            slot = _SlotPool(3 + 3 * len(msrbs), dev, CONV_IMPLS[self.conv_impl] == NS_F16X3)
            s_a, s_b, s_cur = slot(), slot(), slot()
            cur, nxt = (torch.empty(B * 64 * H * W, dtype=torch.float32, device=dev) for _ in range(2))
            call("tsr_stem_fwd", ptr(x), _I(3), _I(0), _I(3), _I(hin), _I(win), _I(10), ptr(w1), ptr(s1), ptr(sh1), ptr(cur),
                 _I(64), _I(0), _I(1), _I(B), ptr(s_a), stream())
            _conv(prof, pc2, cur, 64, 0, nxt, 64, 0, True, B, H, W, amax_in=s_a, amax_out=s_b)
            _conv(prof, pc3, nxt, 64, 0, cur, 64, 0, True, B, H, W, amax_in=s_b, amax_out=s_cur)
            ws = _msrb_workspace(msrbs[0].halves is not None, cur, B * H * W)
            for p in msrbs:
                s_out = slot()
                _run_msrb(p, prof, cur, s_cur, nxt, 64, 0, s_out, ws, slot, B, H, W)
                cur, nxt, s_cur = nxt, cur, s_out
            out = torch.empty(B, 1, H, W, dtype=torch.float32, device=dev)
            call("tsr_head_fwd", ptr(cur), _I(64), _I(64), ptr(wh), ptr(out), _I(1), _I(B), _I(H), _I(W), stream())
            return out


def _to_nchw(t, B, C, HW, ctot, coff):
    if t.dtype == torch.bfloat16:      # bf16-storage probes: plain tensor ops (test plumbing only)
        v = t.view(B, ctot // 16, HW, 16)[:, coff // 16:(coff + C) // 16]
        return v.permute(0, 1, 3, 2).reshape(B * C * HW).float()
    dst = torch.empty(B * C * HW, dtype=torch.float32, device=t.device)
    call("tsr_cb16_to_nchw", ptr(t), ptr(dst), _I(B), _I(C), _I(HW), _I(ctot), _I(coff), stream())
    return dst


def to_cb16(x: torch.Tensor, ctot: Optional[int] = None, coff: int = 0, dst: Optional[torch.Tensor] = None):
    """NCHW (B,C,H,W) -> CB16 flat buffer (test plumbing)."""
    B, C, H, W = x.shape
    ctot = ctot or C
    if dst is None:
        dst = torch.zeros(B * ctot * H * W, dtype=torch.float32, device=x.device)
    call("tsr_nchw_to_cb16", ptr(x.contiguous()), ptr(dst), _I(B), _I(C), _I(H * W), _I(ctot), _I(coff), stream())
    return dst


def from_cb16(t: torch.Tensor, B, C, H, W, ctot: Optional[int] = None, coff: int = 0):
    return _to_nchw(t, B, C, H * W, ctot or C, coff).view(B, C, H, W)
