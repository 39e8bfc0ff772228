#!/usr/bin/env python3
"""Cost of the SSIM loss term (tsr_ssim_fwd_bwd), timed with HIP events:
    python tools/loss_microbench.py [--rounds R] [--only kernel|step] [--steps-of b32_eager] [--out profiles/ssim_loss_cost.json]
Measures
  kernel   the launch alone at (8192,1,40,40) and (256,1,100,100), window 11: values only, with dy (accumulating, as the
           train step calls it), and the MSE launch pair beside it; ms per launch and the HBM bytes the launch has to
           move over that time.
  step     the train step (``train_one_iter``: forward + loss + backward + Adam, train_impl fp16x3, sf 10 / T 1) with
           ssim_loss_weight 0 and 0.1: eager at B = 2048, eager at B = 32, graph-replayed (``GraphedTrainStep``) at B = 32;
           and at B = 32 eager the same loss composed from torch ops through autograd (``torch`` below) -- what a user
           has without the kernel.
Every configuration of one comparison holds its own model from the same seed; all are warmed, then they alternate inside
each of R rounds; reported are the median round and the spread (max - min) in ms, and for the steps the difference to
weight 0 with the run's spread beside it.  Targets are contact-like blobs (the loss term is ~0 on white noise), the
steps run at the reference's warm-up start learning rate, and a case whose output is all zero is marked invalid.

    python tools/loss_microbench.py --pixel-loss [--rounds R] [--out profiles/pixel_loss_cost.json]
times the pixel-loss launch (tsr_pixel_loss_fwd_bwd) instead, at B = 32 and B = 8192 of 1x40x40, in one process: the
launch pair at every kind without and with a contact weight (and with the target gradient), the MSE launch pair
(tsr_mse_fwd_bwd) beside it, both on preallocated buffers, and the same loss with its gradient composed from torch ops
through autograd, the contact mask included.  Sparse contact targets, predictions relu(t + noise).

    python tools/loss_microbench.py --degradation [--rounds R] [--out profiles/degradation_loss_cost.json]
times the degradation-consistency launch (tsr_degrade_fwd_bwd) instead, in one process: the launch on preallocated
buffers at B = 32 and B = 8192 of 1x40x40 and 1x100x100 -- the forward alone, and with q and an accumulating dy as the
train step calls it -- against the same term and its gradient composed from torch ops in fp32 through autograd (the mask
tables prepared once outside the timing; per call two batched matmuls, the mask floor, the residual and the MSE); and
the B = 32 train step, eager and graph-replayed, without the key (the step as it was before the term existed) and with
``degradation_loss_weight`` 0.1.

    python tools/loss_microbench.py --sample-weight [--rounds R] [--out profiles/sample_weight_cost.json]
times the per-sample supervision weights instead, in one process, at B = 32 and B = 8192 of 1x40x40 and 1x100x100 with
the L1 pixel term and the SSIM term (weight 0.1, window 11): the weighted launch set as ``sr_loss_fwd_bwd`` issues it
(tsr_sample_scale, tsr_pixel_loss_ps_fwd_bwd, tsr_ssim_fwd_bwd_ps accumulating, tsr_weighted_mean) with all weights 1
with a random half of the weights 0 and with every second weight 0 (workgroup b takes image b and the hardware deals
workgroups to the eight XCDs in turn, so that pattern leaves four of them idle); the unweighted launch pair of the same call without a weight (tsr_pixel_loss_fwd_bwd +
tsr_ssim_fwd_bwd: the entry points the step had before the weights -- run from this build, not from the parent
commit's binary); the same weighted loss and its gradient composed from torch ops in fp32 through autograd; and the
B = 32 train step, eager and graph-replayed, on a 2-tuple batch and on a 4-tuple batch with all weights 1 and with a
random half of them 0."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import tactilesr_amd  # noqa: E402
import tactilesr_amd.functional as Fh  # noqa: E402
from tactilesr_amd import optim  # noqa: E402
from tactilesr_amd.train import tactileSR_train as TR  # noqa: E402
from tactilesr_amd.train.graph import GraphedTrainStep  # noqa: E402

LR_START = 1e-3 * 1e-4          # the reference's base lr x its warm-up factor: the first iteration's learning rate
WEIGHT = 0.1
KERNEL_SHAPES = ((8192, 40, 40), (256, 100, 100))


def blobs(B, H, W, gen, amp=10.0):
    """(B,1,H,W): three Gaussian blobs per image, the largest pixel at most `amp`."""
    r = torch.arange(H, dtype=torch.float32)[None, :, None]
    c = torch.arange(W, dtype=torch.float32)[None, None, :]
    img = torch.zeros(B, H, W)
    for _ in range(3):
        a = 2 + 8 * torch.rand(B, 1, 1, generator=gen)
        cr, cc = torch.rand(B, 1, 1, generator=gen) * H, torch.rand(B, 1, 1, generator=gen) * W
        s = (0.04 + 0.08 * torch.rand(B, 1, 1, generator=gen)) * max(H, W)
        img = img + a * torch.exp(-((r - cr) ** 2 + (c - cc) ** 2) / (2 * s * s))
    return (img * (amp / img.amax(dim=(1, 2), keepdim=True).clamp_min(amp)))[:, None].contiguous()


def torch_ssim(y, t, window=11, sigma=1.5, data_range=1.0):
    """Windowed SSIM from torch ops in the tensors' dtype (the eager alternative): per-sample values.  The five
    moments go through the separable window as ONE stacked tensor, and the window is applied with ``unfold`` views
    and weighted sums -- torch's own element-wise and reduction kernels, no convolution library -- so the composition
    is about as few launches as torch ops allow."""
    k = torch.arange(window, dtype=torch.float64) - (window - 1) / 2
    g = torch.exp(-k * k / (2 * sigma * sigma))
    g = (g / g.sum()).to(y.dtype).to(y.device)
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    z = torch.cat([y, t, y * y, t * t, y * t], dim=1)                         # (B,5,H,W)
    z = (z.unfold(2, window, 1) * g).sum(-1)                                  # rows:    (B,5,H-w+1,W)
    z = (z.unfold(3, window, 1) * g).sum(-1)                                  # columns: (B,5,H-w+1,W-w+1)
    mx, mt, exx, ett, ext = z.unbind(1)
    sxx, stt, sxt = exx - mx * mx, ett - mt * mt, ext - mx * mt
    S = ((2 * mx * mt + C1) * (2 * sxt + C2)) / ((mx * mx + mt * mt + C1) * (sxx + stt + C2))
    return S.mean(dim=(1, 2))


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def alternate(fns, warmup, rounds, n):
    """{name: [ms per call, one per round]}: every fn warmed, then the fns take turns inside each round."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(timed(fn, n))
    return t


def kernel_cases(a):
    cases = []
    for B, H, W in KERNEL_SHAPES:
        gen = torch.Generator().manual_seed(43)
        t = blobs(B, H, W, gen).cuda()
        y = (t + 0.5 * torch.randn(t.shape, generator=gen).cuda()).clamp_min(0).contiguous()
        dy = torch.zeros_like(y)
        fns = {
            "ssim_values": lambda: Fh._ssim_launch(y, t, 1.0, 11, 1.5, 0.01, 0.03, None, 0.0, 0),
            "ssim_with_dy": lambda: Fh._ssim_launch(y, t, 1.0, 11, 1.5, 0.01, 0.03, dy, -WEIGHT / B, 1),
            "mse_fwd_bwd": lambda: Fh.mse_fwd_bwd(y, t),
        }
        rounds = alternate(fns, a.warmup, a.rounds, a.launches)
        px = B * H * W * 4
        moved = {"ssim_values": 2 * px, "ssim_with_dy": 5 * px, "mse_fwd_bwd": 3 * px}   # y, t (twice with dy: the adjoint rereads them) + dy read and written
        for k, v in rounds.items():
            med = statistics.median(v)
            case = dict(shape=[B, 1, H, W], window=11, launch=k, ms_median=round(med, 5), ms_spread=round(max(v) - min(v), 5),
                        rounds_ms=[round(x, 5) for x in v], bytes_moved=moved[k], gb_per_s=round(moved[k] / med / 1e6, 1))
            cases.append(case)
            print(f"[loss microbench] kernel ({B},1,{H},{W}) {k:13s}: {med:8.4f} ms (spread {case['ms_spread']:.4f}), "
                  f"{case['gb_per_s']:.0f} GB/s of the bytes it has to move", flush=True)
    return cases


PIXEL_BATCHES = (32, 8192)
PIXEL_KINDS = (("mse", None), ("l1", None), ("charbonnier", 1e-3), ("huber", 1.0))
CONTACT = (4.0, 0.5)            # weight, threshold


def torch_pixel(y, t, kind, param, fg_weight, fg_threshold):
    """The loss and d loss / d y from torch ops through autograd (the eager alternative)."""
    yy = y.detach().requires_grad_(True)
    d = yy - t
    if kind == "mse":
        rho = d * d
    elif kind == "l1":
        rho = d.abs()
    elif kind == "charbonnier":
        rho = torch.sqrt(d * d + param * param)
    else:
        a = d.abs()
        rho = torch.where(a <= param, 0.5 * d * d, param * (a - 0.5 * param))
    if fg_weight:
        rho = rho * (1 + fg_weight * (t > fg_threshold))
    loss = rho.mean()
    return loss, torch.autograd.grad(loss, yy)[0]


def pixel_cases(a):
    from tactilesr_amd import _lib
    from tactilesr_amd._lib import c_double, c_float, c_int, c_longlong, ptr, stream
    cases = []
    for B in PIXEL_BATCHES:
        gen = torch.Generator().manual_seed(43)
        shape = (B, 1, 40, 40)
        t = torch.where(torch.rand(shape, generator=gen) < 0.1, 2 * torch.rand(shape, generator=gen), torch.zeros(shape)).cuda()
        y = (t + 0.3 * torch.randn(shape, generator=gen).cuda()).clamp_min(0).contiguous()
        n = y.numel()
        dy, dt = torch.empty_like(y), torch.empty_like(y)
        loss = torch.empty(1, device="cuda")
        work = torch.empty(Fh.PIXEL_LOSS_WORK, dtype=torch.float64, device="cuda")

        def pixel(kind, param, w, thr, with_dt=False):
            _lib.call("tsr_pixel_loss_fwd_bwd", ptr(y), ptr(t), c_longlong(n), c_int(Fh.PIXEL_KINDS[kind]),
                      c_double(param or 0.0), c_float(w), c_float(thr), ptr(loss), ptr(dy), c_float(1.0), c_int(0),
                      ptr(dt if with_dt else None), ptr(work), stream())

        fns = {"mse_fwd_bwd": lambda: _lib.call("tsr_mse_fwd_bwd", ptr(y), ptr(t), ptr(dy), ptr(loss), c_longlong(n),
                                                c_float(1.0), ptr(work), stream())}
        moved = {"mse_fwd_bwd": 3}                                  # tensors read or written: y, t, dy
        for kind, param in PIXEL_KINDS:
            fns[f"pixel_{kind}"] = lambda k=kind, p=param: pixel(k, p, 0.0, 0.0)
            fns[f"pixel_{kind}_contact"] = lambda k=kind, p=param: pixel(k, p, *CONTACT)
            fns[f"torch_{kind}"] = lambda k=kind, p=param: torch_pixel(y, t, k, p, 0.0, 0.0)
            fns[f"torch_{kind}_contact"] = lambda k=kind, p=param: torch_pixel(y, t, k, p, *CONTACT)
            moved[f"pixel_{kind}"] = moved[f"pixel_{kind}_contact"] = 3
        fns["pixel_huber_contact_dt"] = lambda: pixel("huber", 1.0, *CONTACT, with_dt=True)
        moved["pixel_huber_contact_dt"] = 4
        rounds = alternate(fns, a.warmup, a.rounds, a.launches)
        med = {k: statistics.median(v) for k, v in rounds.items()}
        for k, v in rounds.items():
            case = dict(shape=list(shape), launch=k, ms_median=round(med[k], 5), ms_spread=round(max(v) - min(v), 5),
                        rounds_ms=[round(x, 5) for x in v], ratio_to_mse_fwd_bwd=round(med[k] / med["mse_fwd_bwd"], 3))
            if k in moved:
                case.update(bytes_moved=moved[k] * n * 4, gb_per_s=round(moved[k] * n * 4 / med[k] / 1e6, 1))
            cases.append(case)
            print(f"[loss microbench] pixel ({B},1,40,40) {k:26s}: {med[k]:8.4f} ms (spread {case['ms_spread']:.4f}), "
                  f"{case['ratio_to_mse_fwd_bwd']:.2f} x mse_fwd_bwd" +
                  (f", {case['gb_per_s']:.0f} GB/s" if k in moved else ""), flush=True)
    return cases


DEG_SHAPES = ((32, 40, 40), (8192, 40, 40), (32, 100, 100), (8192, 100, 100))
DEG_GAMMA, DEG_GAIN = 0.7, 10.0


def torch_degrade_tables(H, W, gamma, device):
    """(E (4,H), F (4,W), mn, k / gain) in fp32 for `torch_degrade`, evaluated in fp64."""
    KM = 100.0 / 15138.0
    c = 12.0 + 25.0 * torch.arange(4, dtype=torch.float64).view(4, 1)
    tab = [torch.exp(-KM * ((torch.arange(n, dtype=torch.float64) + 0.5) * 100.0 / n - 0.5 - c) ** 2 / gamma) for n in (H, W)]
    mn = float(torch.exp(torch.tensor(-100.0 / gamma, dtype=torch.float64)))
    return tab[0].float().to(device), tab[1].float().to(device), mn, 1e-4 * (100.0 / H) * (100.0 / W) / (1 - mn)


def torch_degrade(y, z, tables, gain):
    """mean_b q_b and its gradient with respect to y from torch ops through autograd (the eager alternative)."""
    E, F, mn, k = tables
    yy = y.detach().requires_grad_(True)
    S = torch.matmul(torch.matmul(E, yy[:, 0]), F.t())                               # (B,4,4): two batched matmuls
    D = (gain * k) * (S - mn * yy.sum(dim=(1, 2, 3)).view(-1, 1, 1))
    loss = ((D - z) ** 2).mean()
    return loss, torch.autograd.grad(loss, yy)[0]


def degradation_cases(a):
    from tactilesr_amd import _lib
    from tactilesr_amd._lib import c_double, c_float, c_int, c_longlong, ptr, stream
    cases = []
    for B, H, W in DEG_SHAPES:
        gen = torch.Generator().manual_seed(43)
        y = blobs(B, H, W, gen, amp=1.0).cuda()
        z = (torch.rand(B, 3, 4, 4, generator=gen) * 8).cuda()
        zc = z[:, 2]                                                # a channel slice, read in place
        zt = zc.contiguous()
        dy, lr_deg, q = torch.zeros_like(y), torch.empty(B, 16, device="cuda"), torch.empty(B, device="cuda")
        tables = torch_degrade_tables(H, W, DEG_GAMMA, "cuda")

        def launch(with_z, with_dy):
            _lib.call("tsr_degrade_fwd_bwd", ptr(y), c_int(B), c_int(H), c_int(W),
                      _lib.c_void_p(zc.data_ptr() if with_z else 0), c_longlong(48), ptr(None), c_double(DEG_GAMMA),
                      c_double(DEG_GAIN), ptr(lr_deg), ptr(q if with_z else None), ptr(dy if with_dy else None),
                      c_float(WEIGHT / B), c_int(1 if with_dy else 0), ptr(None), stream())

        fns = {"degrade_forward": lambda: launch(False, False), "degrade_q": lambda: launch(True, False),
               "degrade_q_dy": lambda: launch(True, True),
               "functional_fwd_bwd": lambda: Fh.degradation_fwd_bwd(y, zc, DEG_GAMMA, DEG_GAIN, dy=dy, dy_scale=WEIGHT / B,
                                                                    accumulate=True),
               "torch_fwd_bwd": lambda: torch_degrade(y, zt, tables, DEG_GAIN)}
        px = B * H * W * 4
        moved = {"degrade_forward": px, "degrade_q": px, "degrade_q_dy": 3 * px}     # y read; dy read and written
        rounds = alternate(fns, a.warmup, a.rounds, a.launches if B <= 32 else max(a.launches // 5, 5))
        med = {k: statistics.median(v) for k, v in rounds.items()}
        for k, v in rounds.items():
            case = dict(shape=[B, 1, H, W], launch=k, ms_median=round(med[k], 5), ms_spread=round(max(v) - min(v), 5),
                        rounds_ms=[round(x, 5) for x in v], ratio_to_torch=round(med[k] / med["torch_fwd_bwd"], 4))
            if k in moved:
                case.update(bytes_moved=moved[k], gb_per_s=round(moved[k] / med[k] / 1e6, 1))
            cases.append(case)
            print(f"[loss microbench] degradation ({B},1,{H},{W}) {k:19s}: {med[k]:8.4f} ms (spread {case['ms_spread']:.4f}), "
                  f"{case['ratio_to_torch']:.3f} x the torch composition" +
                  (f", {case['gb_per_s']:.0f} GB/s" if k in moved else ""), flush=True)
        del y, dy
        torch.cuda.empty_cache()
    return cases


def degradation_step_cases(a):
    """The B = 32 train step, eager and graph-replayed: without the key (the step as it was) and with weight 0.1."""
    cases = []
    B = 32
    gen = torch.Generator().manual_seed(43)
    batch = ((torch.rand(B, 3, 4, 4, generator=gen) * 8).cuda(), (blobs(B, 100, 100, gen) * 10).cuda())
    for mode in ("eager", "graphed"):
        fns, models = {}, {}
        for name in ("no_key", f"weight_{WEIGHT}"):
            m, opt, conf = build(None)
            if name != "no_key":
                conf.update(degradation_loss_weight=WEIGHT, degradation_gamma=DEG_GAMMA)
            models[name] = m
            if mode == "graphed":
                fns[name] = lambda g=GraphedTrainStep(m, opt, conf, warmup=1): g(batch)
            else:
                fns[name] = lambda m=m, opt=opt, conf=conf: TR.train_one_iter(m, opt, batch, conf)
        n = a.steps * 10
        rounds = alternate(fns, max(a.warmup, 3), a.rounds, n)
        med = {k: statistics.median(v) for k, v in rounds.items()}
        run_spread = max(max(v) - min(v) for v in rounds.values())
        for name, v in rounds.items():
            with torch.no_grad():
                models[name].eval()
                frac = float((models[name](batch[0][:8].float()) > 0).float().mean())
                models[name].train()
            case = dict(B=B, mode=mode, loss=name, ms_per_step_median=round(med[name], 4),
                        ms_per_step_spread=round(max(v) - min(v), 4), rounds_ms=[round(x, 4) for x in v],
                        delta_to_no_key_ms=round(med[name] - med["no_key"], 4), run_spread_ms=round(run_spread, 4),
                        steps_per_round=n, out_nonzero_frac=round(frac, 5), valid=bool(frac > 0))
            cases.append(case)
            print(f"[loss microbench] degradation step B={B} {mode:7s} {name:10s}: {med[name]:9.4f} ms/step (spread "
                  f"{case['ms_per_step_spread']:.4f}), {case['delta_to_no_key_ms']:+.4f} ms to no key (run spread "
                  f"{run_spread:.4f})" + ("" if case["valid"] else "  INVALID: the output is all zero"), flush=True)
        del fns, models
        torch.cuda.empty_cache()
    return cases


SW_SHAPES = ((32, 40, 40), (8192, 40, 40), (32, 100, 100), (8192, 100, 100))
SW_KIND = "l1"


def torch_weighted(y, t, w, data_range):
    """The weighted L1 + SSIM loss ("sum" normalisation) and its gradient from torch ops through autograd.  The
    composition has no way to skip a sample: it multiplies by the weight (a NaN target would reach the loss)."""
    yy = y.detach().requires_grad_(True)
    B = y.shape[0]
    s = w * (B / w.sum())
    per = (yy - t).abs().mean(dim=(1, 2, 3)) + WEIGHT * (1 - torch_ssim(yy, t, data_range=data_range))
    loss = (s * per).sum() / B
    return loss, torch.autograd.grad(loss, yy)[0]


def sample_weight_cases(a):
    cases = []
    for B, H, W in SW_SHAPES:
        gen = torch.Generator().manual_seed(43)
        t = blobs(B, H, W, gen).cuda()
        y = (t + 0.5 * torch.randn(t.shape, generator=gen).cuda()).clamp_min(0).contiguous()
        ones = torch.ones(B, device="cuda")
        half = (torch.randperm(B, generator=gen) < B // 2).float().cuda()      # a random half: no pattern in the index
        every_2nd = (torch.arange(B, device="cuda") % 2 == 0).float()          # images 1, 3, 5, ... unlabeled

        def hip(w):
            return Fh.sr_loss_fwd_bwd(y, t, WEIGHT, data_range=10.0, pixel_kind=SW_KIND, sample_weight=w)

        fns = {"unweighted_pair": lambda: hip(None), "weighted_ones": lambda: hip(ones), "weighted_half_zero": lambda: hip(half),
               "weighted_every_2nd_zero": lambda: hip(every_2nd),
               "torch_ones": lambda: torch_weighted(y, t, ones, 10.0), "torch_half_zero": lambda: torch_weighted(y, t, half, 10.0)}
        big = B * H * W > 1 << 22
        rounds = alternate(fns, a.warmup, a.rounds, max(a.launches // 10, 3) if big else a.launches)
        med = {k: statistics.median(v) for k, v in rounds.items()}
        for k, v in rounds.items():
            against = "torch_ones" if k.endswith("ones") else "torch_half_zero" if k.endswith("zero") else None
            case = dict(shape=[B, 1, H, W], launch=k, ms_median=round(med[k], 5), ms_spread=round(max(v) - min(v), 5),
                        rounds_ms=[round(x, 5) for x in v], ratio_to_unweighted_pair=round(med[k] / med["unweighted_pair"], 4))
            if against and not k.startswith("torch"):
                case.update(ratio_to_torch=round(med[k] / med[against], 4), slower_than_torch=bool(med[k] > med[against]))
            cases.append(case)
            print(f"[loss microbench] sample weight ({B},1,{H},{W}) {k:23s}: {med[k]:9.4f} ms (spread {case['ms_spread']:.4f}), "
                  f"{case['ratio_to_unweighted_pair']:.3f} x the unweighted pair" +
                  (f", {case['ratio_to_torch']:.3f} x the torch composition" if "ratio_to_torch" in case else ""), flush=True)
        del y, t
        torch.cuda.empty_cache()
    return cases


def sample_weight_step_cases(a):
    """The B = 32 train step (L1 + SSIM), eager and graph-replayed: a 2-tuple batch, and a 4-tuple with all weights 1 and
    with a random half of them 0."""
    cases = []
    B = 32
    gen = torch.Generator().manual_seed(43)
    LR, HR = (torch.rand(B, 3, 4, 4, generator=gen) * 8).cuda(), (blobs(B, 100, 100, gen) * 10).cuda()
    batches = {"no_weight": (LR, HR), "weights_one": (LR, HR, None, torch.ones(B, device="cuda")),
               "weights_half_zero": (LR, HR, None, (torch.randperm(B, generator=gen) < B // 2).float().cuda())}
    for mode in ("eager", "graphed"):
        fns, models = {}, {}
        for name, batch in batches.items():
            m, opt, conf = build(WEIGHT)
            conf["pixel_loss"] = SW_KIND
            models[name] = m
            if mode == "graphed":
                fns[name] = lambda g=GraphedTrainStep(m, opt, conf, warmup=1), b=batch: g(b)
            else:
                fns[name] = lambda m=m, opt=opt, conf=conf, b=batch: TR.train_one_iter(m, opt, b, conf)
        n = a.steps * 10
        rounds = alternate(fns, max(a.warmup, 3), a.rounds, n)
        med = {k: statistics.median(v) for k, v in rounds.items()}
        run_spread = max(max(v) - min(v) for v in rounds.values())
        for name, v in rounds.items():
            with torch.no_grad():
                models[name].eval()
                frac = float((models[name](LR[:8].float()) > 0).float().mean())
                models[name].train()
            case = dict(B=B, mode=mode, batch=name, ms_per_step_median=round(med[name], 4),
                        ms_per_step_spread=round(max(v) - min(v), 4), rounds_ms=[round(x, 4) for x in v],
                        delta_to_no_weight_ms=round(med[name] - med["no_weight"], 4), run_spread_ms=round(run_spread, 4),
                        steps_per_round=n, out_nonzero_frac=round(frac, 5), valid=bool(frac > 0))
            cases.append(case)
            print(f"[loss microbench] sample weight step B={B} {mode:7s} {name:17s}: {med[name]:9.4f} ms/step (spread "
                  f"{case['ms_per_step_spread']:.4f}), {case['delta_to_no_weight_ms']:+.4f} ms to no weight (run spread "
                  f"{run_spread:.4f})" + ("" if case["valid"] else "  INVALID: the output is all zero"), flush=True)
        del fns, models
        torch.cuda.empty_cache()
    return cases


def build(weight):
    torch.manual_seed(42)
    m = tactilesr_amd.TactileSR().cuda().train()
    m.train_impl = "fp16x3"
    opt = optim.Adam(m.parameters(), lr=LR_START, weight_decay=1e-2)
    conf = dict(TR.default_config(), ssim_data_range=10.0)
    if weight is not None:
        conf["ssim_loss_weight"] = weight
    return m, opt, conf


def torch_step(m, opt, batch, conf):
    """train_one_iter with the SSIM term composed from torch ops (fp32) through autograd."""
    LR, HR = TR._prep(batch, conf, "cuda")
    out = m(LR)
    loss = Fh.mse_loss(out, HR) + WEIGHT * (1 - torch_ssim(out, HR, data_range=conf["ssim_data_range"]).mean())
    opt.zero_grad()
    loss.backward()
    opt.step()
    return {"total_loss": loss}


def step_cases(a):
    cases = []
    for B, modes in ((2048, ("eager",)), (32, ("eager", "graphed"))):
        modes = [mode for mode in modes if a.steps_of in (None, f"b{B}_{mode}")]
        if not modes:
            continue
        gen = torch.Generator().manual_seed(43)
        batch = ((torch.rand(B, 3, 4, 4, generator=gen) * 8).cuda(), (blobs(B, 100, 100, gen) * 10).cuda())
        for mode in modes:
            names = ["weight_0", f"weight_{WEIGHT}"] + (["torch"] if (B, mode) == (32, "eager") else [])
            fns, models = {}, {}
            for name in names:
                m, opt, conf = build(None if name == "weight_0" else (0.0 if name == "torch" else WEIGHT))
                models[name] = m
                if name == "torch":
                    fns[name] = lambda m=m, opt=opt, conf=conf: torch_step(m, opt, batch, conf)
                elif mode == "graphed":
                    fns[name] = lambda g=GraphedTrainStep(m, opt, conf, warmup=1): g(batch)
                else:
                    fns[name] = lambda m=m, opt=opt, conf=conf: TR.train_one_iter(m, opt, batch, conf)
            n = a.steps if B > 32 else a.steps * 10
            rounds = alternate(fns, max(a.warmup, 3), a.rounds, n)
            med = {k: statistics.median(v) for k, v in rounds.items()}
            run_spread = max(max(v) - min(v) for v in rounds.values())
            for name in names:
                with torch.no_grad():
                    models[name].eval()
                    frac = float((models[name](batch[0][:8].float()) > 0).float().mean())
                    models[name].train()
                v = rounds[name]
                case = dict(B=B, mode=mode, loss=name, ms_per_step_median=round(med[name], 4),
                            ms_per_step_spread=round(max(v) - min(v), 4), rounds_ms=[round(x, 4) for x in v],
                            delta_to_weight_0_ms=round(med[name] - med["weight_0"], 4), run_spread_ms=round(run_spread, 4),
                            steps_per_round=n, out_nonzero_frac=round(frac, 5), valid=bool(frac > 0))
                cases.append(case)
                print(f"[loss microbench] step B={B} {mode:7s} {name:10s}: {med[name]:9.4f} ms/step (spread "
                      f"{case['ms_per_step_spread']:.4f}), {case['delta_to_weight_0_ms']:+.4f} ms to weight 0 (run spread "
                      f"{run_spread:.4f})" + ("" if case["valid"] else "  INVALID: the output is all zero"), flush=True)
            del fns, models
            torch.cuda.empty_cache()
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50, help="kernel launches per round")
    ap.add_argument("--steps", type=int, default=5, help="train steps per round at B = 2048 (ten times as many at B = 32)")
    ap.add_argument("--only", choices=("kernel", "step"), default=None)
    ap.add_argument("--steps-of", choices=("b2048_eager", "b32_eager", "b32_graphed"), default=None,
                    help="time only this step comparison")
    ap.add_argument("--pixel-loss", action="store_true", help="time the pixel-loss launch instead (see the docstring)")
    ap.add_argument("--degradation", action="store_true", help="time the degradation launch and its step instead (see "
                                                               "the docstring)")
    ap.add_argument("--sample-weight", action="store_true", help="time the per-sample weight launches and their step instead "
                                                                 "(see the docstring)")
    ap.add_argument("--out", default=None, help="default: profiles/ssim_loss_cost.json, profiles/pixel_loss_cost.json "
                                                "with --pixel-loss, profiles/degradation_loss_cost.json with --degradation, "
                                                "profiles/sample_weight_cost.json with --sample-weight")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(REPO, "profiles", "sample_weight_cost.json" if a.sample_weight else
                             "degradation_loss_cost.json" if a.degradation else
                             "pixel_loss_cost.json" if a.pixel_loss else "ssim_loss_cost.json")
    if not torch.cuda.is_available():
        raise SystemExit("loss_microbench: needs a ROCm device (the timing is of the GPU)")
    result = dict(tool="tools/loss_microbench.py", device=torch.cuda.get_device_name(0), rounds=a.rounds, warmup=a.warmup,
                  launches=a.launches, steps=a.steps, weight=WEIGHT, lr=LR_START)
    if a.sample_weight:
        import datetime
        result = dict(tool="tools/loss_microbench.py --sample-weight", device=result["device"],
                      date=datetime.date.today().isoformat(), rounds=a.rounds, warmup=a.warmup, launches=a.launches,
                      steps=a.steps, ssim_weight=WEIGHT, pixel_loss=SW_KIND, lr=LR_START, norm="sum",
                      not_measured=["the parent commit's own binary: unweighted_pair and no_weight are this build's "
                                    "unweighted entry points"],
                      launch=sample_weight_cases(a), step=sample_weight_step_cases(a))
    elif a.degradation:
        result = dict(tool="tools/loss_microbench.py --degradation", device=result["device"], rounds=a.rounds,
                      warmup=a.warmup, launches=a.launches, steps=a.steps, weight=WEIGHT, gamma=DEG_GAMMA, gain=DEG_GAIN,
                      lr=LR_START, launch=degradation_cases(a), step=degradation_step_cases(a))
    elif a.pixel_loss:
        result = dict(tool="tools/loss_microbench.py --pixel-loss", device=result["device"], rounds=a.rounds,
                      warmup=a.warmup, launches=a.launches, contact_weight=CONTACT[0], contact_threshold=CONTACT[1],
                      pixel=pixel_cases(a))
    else:
        if a.only != "step":
            result["kernel"] = kernel_cases(a)
        if a.only != "kernel":
            result["step"] = step_cases(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"[loss microbench] wrote {a.out}")


if __name__ == "__main__":
    main()
