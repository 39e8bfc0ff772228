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
bytes a batch has to move (read + write of both tensors, index and ops) over that time."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "augment_cost.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_microbench needs a ROCm device: a CPU timing says nothing about the kernel")
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
