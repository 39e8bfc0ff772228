"""Shared by tests/test_gpu_workspace_poison.py and tests/test_gpu_call_history.py: the full result of an engine call as
{name: tensor} -- outputs, gradients, parameters, buffers, optimizer and EMA state -- and seeded TactileSR modules."""
import torch

import tactilesr_amd


def bits(t):
    t = t.detach().cpu().reshape(-1).contiguous()
    return t.view(torch.uint8) if t.is_floating_point() and t.numel() else t


def as_results(d):
    out = {}
    for k, v in d.items():
        if v is None:
            continue
        if not isinstance(v, torch.Tensor):
            v = torch.as_tensor(v, dtype=torch.float64)
        out[k] = v.detach().clone()
    return out


def cfg_of(T, M, R, sf=3):
    return dict(scale_factor=sf, seqsCnt=T, patternFeatureExtraLayerCnt=M, forceFeatureExtraLayerCnt=R)


def tsr_model(cfg, sd, **attrs):
    m = tactilesr_amd.TactileSR(**cfg)
    m.load_state_dict(sd, strict=True)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m.cuda()


def model_state(m):
    d = {}
    for n, p in m.named_parameters():
        d["param:" + n] = p
        if p.grad is not None:
            d["grad:" + n] = p.grad
    for n, b in m.named_buffers():
        d["buf:" + n] = b
    return d


def opt_state(opt, m):
    d = {}
    for n, p in m.named_parameters():
        for k, v in opt.state.get(p, {}).items():
            d[f"opt:{n}.{k}"] = v if isinstance(v, torch.Tensor) else float(v)
    return d


def ema_state(e):
    d = {"ema:" + k: v for k, v in e.shadow.items()}
    d["ema_updates"] = float(e.updates)
    return d


def same_results(got, want, label=""):
    """Every tensor of `got` equals its twin in `want` (`torch.equal`: values, so a NaN anywhere fails) and is finite."""
    got, want = as_results(got), as_results(want)
    assert list(got) == list(want), (label, sorted(set(got) ^ set(want)))
    bad = []
    for k, w in want.items():
        g = got[k]
        if g.shape != w.shape or g.dtype != w.dtype or not torch.equal(g.cpu(), w.cpu()):
            bad.append(k)
        elif g.is_floating_point() and not bool(torch.isfinite(g).all()):
            bad.append(k + " (not finite)")
    assert not bad, f"{label}: differs from the fresh object in {len(bad)} of {len(want)} results: {bad[:8]}"


def fresh_like(m):
    """A newly constructed module of `m`'s class with `m`'s state, arithmetic attributes, BatchNorm eps / modes and
    `requires_grad` flags, on `m`'s device: what `m` would be had it never been called."""
    if isinstance(m, tactilesr_amd.TactileSR):
        f = tactilesr_amd.TactileSR(m.scale_factor, m.seqsCnt, m.axisCnt, len(m.patternFeatureExtra_layer),
                                    len(m.forceFeatureExtra_layer))
    else:
        f = type(m)()
    f.load_state_dict({k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, strict=True)
    for a in ("conv_impl", "train_impl", "head_impl", "fuse_1x1", "fuse_pair", "max_images_per_pass"):
        if hasattr(m, a):
            setattr(f, a, getattr(m, a))
    f = f.to(next(m.parameters()).device)
    f.train(m.training)
    for (_, a), (_, b) in zip(m.named_modules(), f.named_modules()):
        if isinstance(a, torch.nn.BatchNorm2d):
            b.eps, b.momentum, b.training = a.eps, a.momentum, a.training
    for (_, p), (_, q) in zip(m.named_parameters(), f.named_parameters()):
        q.requires_grad_(p.requires_grad)
    return f
