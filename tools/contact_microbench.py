#!/usr/bin/env python3
"""Cost of the contact readout (tsr_contact_readout), timed with HIP events:
    python tools/contact_microbench.py [--rounds R] [--out profiles/contact_readout_cost.json]
Measures, in one process,
  launch   the pair launch through ``functional.contact_metrics`` (which allocates its three outputs) and through the raw
           entry point on preallocated buffers, and the single form through ``functional.contact_readout``, at B = 8192
           and B = 32 of 1x40x40 and 1x100x100 -- against the same readout composed from torch ops in fp32 on the same
           device (``torch_pair`` / ``torch_single``: threshold, coordinate grids prepared once outside the timing, masked
           sums, argmax, atan2, the eigenvalues, the set counts; nothing is read back);
  sensor   ``functional.sr_readout`` (the eval forward plus the launch) against the plain eval forward, and against the
           forward followed by the torch composition, at B = 8, the reference's eval batch.
All cases of one comparison are warmed, then they alternate inside each of R rounds; reported are the median round and
the spread (max - min) in ms.  Images are contact-like blobs; the threshold is the reference's rule ("range", 0.5)."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import tactilesr_amd  # noqa: E402
import tactilesr_amd.functional as Fh  # noqa: E402
from loss_microbench import alternate, blobs  # noqa: E402

SHAPES = ((8192, 40, 40), (32, 40, 40), (8192, 100, 100), (32, 100, 100))
MODE, THRESHOLD, GAIN, SPAN = "range", 0.5, 10.0, (4.0, 4.0)


def torch_grids(H, W, device):
    u = ((torch.arange(H, dtype=torch.float32, device=device) + 0.5) * SPAN[0] / H - 0.5)
    v = ((torch.arange(W, dtype=torch.float32, device=device) + 0.5) * SPAN[1] / W - 0.5)
    return u.repeat_interleave(W)[None], v.repeat(H)[None]


def torch_single(y, grids):
    """The 16 entries of the record from torch ops, fp32, batched; returns (record (B,16), mask)."""
    U, V = grids
    f = y.flatten(1)
    mn, mx = f.amin(1), f.amax(1)
    tau = mn + THRESHOLD * (mx - mn)
    m = f > tau[:, None]
    w = f * m
    n = m.sum(1).float()
    M0 = w.sum(1)
    first = f.argmax(1)
    cu, cv = (w * U).sum(1) / M0, (w * V).sum(1) / M0
    du, dv = U - cu[:, None], V - cv[:, None]
    muu, mvv, muv = (w * du * du).sum(1) / M0, (w * dv * dv).sum(1) / M0, (w * du * dv).sum(1) / M0
    th = 0.5 * torch.atan2(2 * muv, muu - mvv)
    h, d = 0.5 * (muu + mvv), torch.sqrt((0.5 * (muu - mvv)) ** 2 + muv * muv)
    H, W = y.shape[-2:]
    rec = torch.stack([n, n * (SPAN[0] / H * SPAN[1] / W), GAIN * M0, GAIN * f.sum(1), GAIN * mx, U[0][first], V[0][first],
                       cu, cv, muu, mvv, muv, th, (h + d).clamp_min(0).sqrt(), (h - d).clamp_min(0).sqrt(), tau], dim=1)
    return rec, m


def torch_pair(y, t, grids):
    ry, my = torch_single(y, grids)
    rt, mt = torch_single(t, grids)
    inter = (my & mt).sum(1).float()
    uni = ry[:, 0] + rt[:, 0] - inter
    dth = (ry[:, 12] - rt[:, 12]).abs()
    pair = torch.stack([inter, uni, torch.where(uni > 0, inter / uni, torch.ones_like(uni)),
                        torch.where(ry[:, 0] + rt[:, 0] > 0, 2 * inter / (ry[:, 0] + rt[:, 0]), torch.ones_like(uni)),
                        torch.hypot(ry[:, 7] - rt[:, 7], ry[:, 8] - rt[:, 8]), (ry[:, 2] - rt[:, 2]).abs() / rt[:, 2],
                        torch.hypot(ry[:, 5] - rt[:, 5], ry[:, 6] - rt[:, 6]),
                        torch.where(dth > torch.pi / 2, torch.pi - dth, dth)], dim=1)
    return pair, ry, rt


def _case(rounds, med, ref, **head):
    out = []
    for k, v in rounds.items():
        out.append(dict(**head, launch=k, ms_median=round(med[k], 5), ms_spread=round(max(v) - min(v), 5),
                        rounds_ms=[round(x, 5) for x in v], ratio_to_torch=round(med[k] / med[ref[k]], 4)))
    return out


def launch_cases(a):
    from tactilesr_amd import _lib
    from tactilesr_amd._lib import c_double, c_int, ptr, stream
    cases = []
    for B, H, W in SHAPES:
        gen = torch.Generator().manual_seed(43)
        t = blobs(B, H, W, gen, amp=1.0).cuda()
        y = (t + 0.05 * torch.randn(t.shape, generator=gen).cuda()).clamp_min(0).contiguous()
        grids = torch_grids(H, W, "cuda")
        rec = torch.empty(2, B, Fh.CONTACT_REC, device="cuda")
        pair = torch.empty(B, Fh.CONTACT_PAIR, device="cuda")

        def raw():
            _lib.call("tsr_contact_readout", ptr(y), ptr(t), c_int(B), c_int(H), c_int(W), c_int(Fh.CONTACT_MODES[MODE]),
                      c_double(THRESHOLD), c_double(GAIN), c_double(SPAN[0]), c_double(SPAN[1]), ptr(rec[0]), ptr(rec[1]),
                      ptr(pair), stream())

        fns = {"pair_raw": raw, "contact_metrics": lambda: Fh.contact_metrics(y, t, THRESHOLD, MODE, GAIN, SPAN),
               "torch_pair": lambda: torch_pair(y, t, grids),
               "contact_readout": lambda: Fh.contact_readout(y, THRESHOLD, MODE, GAIN, SPAN),
               "torch_single": lambda: torch_single(y, grids)}
        ref = {"pair_raw": "torch_pair", "contact_metrics": "torch_pair", "torch_pair": "torch_pair",
               "contact_readout": "torch_single", "torch_single": "torch_single"}
        got, want = Fh.contact_metrics(y, t, THRESHOLD, MODE, GAIN, SPAN)[0].raw, torch_pair(y, t, grids)[0]
        agree = float((got[:, 2] - want[:, 2]).abs().max())         # the two sides compute the same thing
        rounds = alternate(fns, a.warmup, a.rounds, a.launches if B <= 32 else max(a.launches // 5, 5))
        med = {k: statistics.median(v) for k, v in rounds.items()}
        new = _case(rounds, med, ref, shape=[B, 1, H, W])
        px = 2 * B * H * W * 4
        for c in new:
            if c["launch"] in ("pair_raw", "contact_metrics"):
                c.update(bytes_read_once=px, gb_per_s=round(px / c["ms_median"] / 1e6, 1))
            c["iou_max_abs_diff_to_torch"] = round(agree, 7)
            print(f"[contact microbench] ({B},1,{H},{W}) {c['launch']:16s}: {c['ms_median']:8.4f} ms (spread "
                  f"{c['ms_spread']:.4f}), {c['ratio_to_torch']:.3f} x its torch composition", flush=True)
        cases += new
        del y, t
        torch.cuda.empty_cache()
    return cases


def sensor_cases(a):
    B = 8
    torch.manual_seed(42)
    m = tactilesr_amd.TactileSR().cuda().eval()
    gen = torch.Generator().manual_seed(43)
    LR = (torch.rand(B, 3, 4, 4, generator=gen) * 8).cuda()
    with torch.no_grad():
        H, W = m(LR).shape[-2:]
    grids = torch_grids(H, W, "cuda")

    @torch.no_grad()
    def forward():
        return m(LR)

    @torch.no_grad()
    def forward_torch():
        return torch_single(m(LR), grids)

    fns = {"forward": forward, "sr_readout": lambda: Fh.sr_readout(m, LR, threshold=THRESHOLD, mode=MODE, gain=GAIN),
           "forward_plus_torch": forward_torch}
    rounds = alternate(fns, max(a.warmup, 3), a.rounds, a.launches)
    med = {k: statistics.median(v) for k, v in rounds.items()}
    cases = []
    for k, v in rounds.items():
        c = dict(B=B, shape=[B, 1, H, W], call=k, ms_median=round(med[k], 5), ms_spread=round(max(v) - min(v), 5),
                 rounds_ms=[round(x, 5) for x in v], delta_to_forward_ms=round(med[k] - med["forward"], 5))
        cases.append(c)
        print(f"[contact microbench] sensor loop B={B} {k:18s}: {med[k]:8.4f} ms (spread {c['ms_spread']:.4f}), "
              f"{c['delta_to_forward_ms']:+.4f} ms to the forward", flush=True)
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "contact_readout_cost.json"))
    a = ap.parse_args()
    res = dict(tool="tools/contact_microbench.py", device=torch.cuda.get_device_name(0), rounds=a.rounds, warmup=a.warmup,
               launches=a.launches, mode=MODE, threshold=THRESHOLD, gain=GAIN, span=list(SPAN),
               launch=launch_cases(a), sensor=sensor_cases(a))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"[contact microbench] wrote {a.out}")


if __name__ == "__main__":
    main()
