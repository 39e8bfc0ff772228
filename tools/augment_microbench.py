#!/usr/bin/env python3
"""Cost of the rot90 / flip augmentation on the device (tsr_gather_dihedral), timed with HIP events:
    python tools/augment_microbench.py [--rounds R] [--launches L] [--out profiles/augment_cost.json]
For the tPSFNet pair (3,4,4) + (100,100) and the SR pair (3,4,4) + (1,100,100), at B = 8192 and B = 32 out of a
device-resident set of as many samples, one batch of a shuffled epoch is produced by
  index_select   plain ``index_select`` of both tensors: today's loader, no augmentation;
  fused          ``functional.dihedral`` with one random op of the eight per sample: one launch per tensor;
  torch_grouped  the same batch composed from torch ops the direct way: per op, the samples that drew it are found with
                 a boolean mask (a host synchronisation each), gathered, flipped / turned and scattered into the batch;
  torch_gather   the same batch without a host round trip: ``index_select``, then ``gather`` through a per-sample
                 element index (an int64 tensor the size of the batch, built from the ops) -- three passes.
The three augmenting forms are checked to give the same bits before anything is timed.  All forms are warmed, then
they alternate inside each of R rounds of L batches; reported are the median round and the spread (max - min) in ms
per batch, for the pair and for its large tensor alone, the ratio to ``index_select``, and for the single-pass forms the
bytes a batch has to move (read + write of both tensors, index and ops) over that time.

    python tools/augment_microbench.py --noise [--rounds R] [--launches L] [--out profiles/taxel_noise_cost.json]
measures the taxel sensor-noise launch (tsr_taxel_noise) instead, the same way: see ``noise_main``."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import tactilesr_amd.functional as Fh  # noqa: E402

PAIRS = {"tpsf": ((3, 4, 4), (100, 100)), "sr": ((3, 4, 4), (1, 100, 100))}
BATCHES = (8192, 32)


def plane_op(x, op):
    if op >= 4:
        x = x.flip(-1)
    return torch.rot90(x, op % 4, (-2, -1))


def element_index(H, W, device):
    """(8, H*W) int64: for each op, the flat source element of every output element (built with the torch ops)."""
    base = torch.arange(H * W, device=device).view(H, W)
    return torch.stack([plane_op(base, op).reshape(-1) for op in range(8)])


def torch_grouped(x, idx, ops):
    out = torch.empty((idx.shape[0],) + x.shape[1:], dtype=x.dtype, device=x.device)
    for op in range(8):
        sel = (ops == op).nonzero().squeeze(1)                      # host sync: the size of the group
        if sel.numel():
            out[sel] = plane_op(x.index_select(0, idx[sel]), op)
    return out


def torch_gather(x, idx, ops, table):
    g = x.index_select(0, idx)
    flat = g.reshape(g.shape[0], -1, table.shape[1])                # (B, planes, H*W)
    index = table[ops.long()].unsqueeze(1).expand_as(flat)
    return flat.gather(2, index).view_as(g)


def time_forms(forms, rounds, launches, warmup):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            start.record()
            for _ in range(launches):
                fn()
            stop.record()
            stop.synchronize()
            ms[k].append(start.elapsed_time(stop) / launches)
    return ms


NOISE_SHAPES = ((3, 4, 4), (21, 4, 4))
NOISE_B = 8192
NOISE_SPEC = dict(sigma_add=0.02, sigma_mul=0.05, gain_jitter=0.1, drop_prob=0.05, drop_value=0.0)


def torch_noise(x, spec, axis_cnt=3):
    """The degradation of ``functional.taxel_noise`` composed from torch ops with torch's global generator: a gain per
    physical taxel, heteroscedastic Gaussian noise, dead taxels."""
    B, C, H, W = x.shape
    v = x.view(B, C // axis_cnt, axis_cnt, H * W)
    gain = torch.rand(B, 1, axis_cnt, H * W, device=x.device) * (2 * spec["gain_jitter"]) + (1 - spec["gain_jitter"])
    v = v * gain
    s = torch.sqrt(spec["sigma_add"] ** 2 + (spec["sigma_mul"] * v) ** 2)
    y = v + s * torch.randn_like(v)
    dead = torch.rand(B, 1, 1, H * W, device=x.device) < spec["drop_prob"]
    return torch.where(dead, spec["drop_value"], y).view(B, C, H, W)


def noise_main(a):
    """--noise: the taxel sensor-noise launch at B = 8192 on the (3,4,4) and (21,4,4) taxels -- back to back, in place, and
    inside a loader batch (one shuffled batch of the whole set, with and without noise, plain and dihedral) -- against the
    same degradation composed from torch ops, all forms alternating inside every round."""
    from tactilesr_amd.data import DeviceSRLoader
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1)
    spec = Fh.TaxelNoise(**NOISE_SPEC)
    rows, B = [], NOISE_B
    for shape in NOISE_SHAPES:
        x = torch.rand((B,) + shape, generator=g, device=dev) * 2 - 1
        hr = torch.rand(B, 1, 40, 40, generator=g, device=dev)
        out, inplace = torch.empty_like(x), x.clone()
        ids = torch.randperm(B, generator=g, device=dev)
        ref = Fh.taxel_noise(x, spec, 1, 1, ids=ids)
        tor = torch_noise(x, NOISE_SPEC)
        assert ref.shape == tor.shape and bool(torch.isfinite(ref).all()) and bool(torch.isfinite(tor).all())
        # the two draw from different generators: the same degradation in distribution (spread of y - x, dead share)
        alive_r, alive_t = ref != 0, tor != 0
        assert abs(float((ref - x)[alive_r].std()) / float((tor - x)[alive_t].std()) - 1) < 0.05
        assert abs(float((~alive_r).float().mean()) - float((~alive_t).float().mean())) < 0.01
        loaders = {
            "loader_plain": DeviceSRLoader(x, hr, B, shuffle=True, seed=1),
            "loader_noise": DeviceSRLoader(x, hr, B, shuffle=True, seed=1, taxel_noise=spec),
            "loader_dihedral": DeviceSRLoader(x, hr, B, shuffle=True, seed=1, augment="dihedral"),
            "loader_dihedral_noise": DeviceSRLoader(x, hr, B, shuffle=True, seed=1, augment="dihedral", taxel_noise=spec),
        }
        step = [0]

        def launch():
            step[0] += 1
            return Fh.taxel_noise(x, spec, 1, step[0], ids=ids, out=out)
        forms = {
            "launch": launch,
            "launch_id_base": lambda: Fh.taxel_noise(x, spec, 1, 1, id_base=0, out=out),
            "launch_in_place": lambda: Fh.taxel_noise(inplace, spec, 1, 1, ids=ids, out=inplace),
            "launch_neutral": lambda: Fh.taxel_noise(x, None, 1, 1, ids=ids, out=out),
            "torch_composed": lambda: torch_noise(x, NOISE_SPEC),
            "torch_copy": lambda: out.copy_(x),
        }
        forms.update({k: (lambda ld=ld: [b for b in ld]) for k, ld in loaders.items()})
        ms = time_forms(forms, a.rounds, a.launches, a.warmup)
        base = statistics.median(ms["torch_composed"])
        nbytes = 2 * 4 * x.numel() + 8 * B
        for k, v in ms.items():
            med = statistics.median(v)
            row = dict(shape=list(shape), B=B, form=k, ms_median=round(med, 5), ms_spread=round(max(v) - min(v), 5),
                       rounds_ms=[round(t, 5) for t in v], ratio_to_torch_composed=round(med / base, 3))
            if k.startswith("launch"):
                row.update(bytes_moved=nbytes, gb_per_s=round(nbytes / med / 1e6, 1))
            rows.append(row)
            print(json.dumps({k2: row[k2] for k2 in ("shape", "form", "ms_median", "ms_spread", "ratio_to_torch_composed")}),
                  flush=True)
        worst_launch, best_torch = max(ms["launch"]), min(ms["torch_composed"])
        rows.append(dict(shape=list(shape), B=B, form="expectation", launch_no_slower_than_torch=bool(worst_launch <= best_torch),
                         launch_worst_round_ms=round(worst_launch, 5), torch_best_round_ms=round(best_torch, 5),
                         loader_noise_extra_ms=round(statistics.median(ms["loader_noise"]) - statistics.median(ms["loader_plain"]), 5),
                         loader_dihedral_noise_extra_ms=round(statistics.median(ms["loader_dihedral_noise"])
                                                              - statistics.median(ms["loader_dihedral"]), 5)))
        print(json.dumps(rows[-1]), flush=True)
    from tactilesr_amd import build
    doc = dict(tool="tools/augment_microbench.py --noise", device=torch.cuda.get_device_name(0), rounds=a.rounds, warmup=a.warmup,
               launches=a.launches, spec=NOISE_SPEC, source_hash=build.source_hash(), rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--noise", action="store_true", help="measure the taxel sensor-noise launch instead (default --out: "
                    "profiles/taxel_noise_cost.json)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(REPO, "profiles", "taxel_noise_cost.json" if a.noise else "augment_cost.json")
    if not torch.cuda.is_available():
        raise SystemExit("augment_microbench needs a ROCm device: a CPU timing says nothing about the kernel")
    if a.noise:
        return noise_main(a)
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1)
    rows = []
    for pair, (s_small, s_large) in PAIRS.items():
        for B in BATCHES:
            small = torch.rand((B,) + s_small, generator=g, device=dev)
            large = torch.rand((B,) + s_large, generator=g, device=dev)
            idx = torch.randperm(B, generator=g, device=dev)
            ops = torch.randint(0, 8, (B,), generator=g, device=dev).to(torch.int32)
            t_small, t_large = element_index(4, 4, dev), element_index(100, 100, dev)
            for x, t in ((small, t_small), (large, t_large)):       # the three forms agree, bit for bit
                ref = Fh.dihedral(x, ops, idx).view(torch.int32)
                assert torch.equal(ref, torch_grouped(x, idx, ops).view(torch.int32))
                assert torch.equal(ref, torch_gather(x, idx, ops, t).view(torch.int32))
            o_small, o_large = torch.empty_like(small), torch.empty_like(large)
            scopes = {
                "pair": {
                    "index_select": lambda: (small.index_select(0, idx), large.index_select(0, idx)),
                    "fused": lambda: (Fh.dihedral(small, ops, idx, out=o_small), Fh.dihedral(large, ops, idx, out=o_large)),
                    "torch_grouped": lambda: (torch_grouped(small, idx, ops), torch_grouped(large, idx, ops)),
                    "torch_gather": lambda: (torch_gather(small, idx, ops, t_small), torch_gather(large, idx, ops, t_large)),
                },
                "large": {
                    "index_select": lambda: large.index_select(0, idx),
                    "index_select_out": lambda: torch.index_select(large, 0, idx, out=o_large),
                    "fused": lambda: Fh.dihedral(large, ops, idx, out=o_large),
                    "fused_identity": lambda: Fh.dihedral(large, None, idx, out=o_large),
                },
            }
            for scope, forms in scopes.items():
                ms = time_forms(forms, a.rounds, a.launches, a.warmup)
                base = statistics.median(ms["index_select"])
                nbytes = 2 * 4 * (large.numel() + (small.numel() if scope == "pair" else 0)) + 12 * B
                for k, v in ms.items():
                    med = statistics.median(v)
                    row = dict(pair=pair, B=B, scope=scope, form=k, ms_median=round(med, 5),
                               ms_spread=round(max(v) - min(v), 5), rounds_ms=[round(x, 5) for x in v],
                               ratio_to_index_select=round(med / base, 3))
                    if not k.startswith("torch"):
                        row.update(bytes_moved=nbytes, gb_per_s=round(nbytes / med / 1e6, 1))
                    rows.append(row)
                    print(json.dumps({k2: row[k2] for k2 in ("pair", "B", "scope", "form", "ms_median", "ms_spread",
                                                             "ratio_to_index_select")}), flush=True)
    from tactilesr_amd import build
    doc = dict(tool="tools/augment_microbench.py", device=torch.cuda.get_device_name(0), rounds=a.rounds, warmup=a.warmup,
               launches=a.launches, ops="dihedral (8), one drawn per sample", source_hash=build.source_hash(), rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
