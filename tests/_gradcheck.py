"""Gradient parity on the activation pattern the device took (helper of the -m gpu training tests).

Why: the network's loss is piecewise linear-ish in every ReLU, so its gradient is DISCONTINUOUS where a
pre-activation is zero to rounding.  Two faithful fp32 forwards (the reference's CPU run, this HIP path, an fp64
run) disagree on the sign of a handful of such pre-activations per batch, and each disagreement moves whole rows of
weight-gradient entries by ~1e-3 of the tensor max.  A max-norm bar against a gradient evaluated on a DIFFERENT
activation pattern therefore cannot be tight, and a loose one hides real kernel bugs.

So the tests do both halves explicitly:
  1. pattern check -- the HIP masks equal the fp64 oracle's own masks except at elements whose fp64 pre-activation
     is within `flip_tol` (relative to that tensor's max) of zero; the count of such flips is reported and bounded;
  2. gradient check -- the fp64 oracle gradient is re-evaluated ON the HIP masks (oracle.ReluTap), and every
     parameter gradient of the HIP path must match it in max-norm (relative to the tensor's max) to `tol`.
"""
import torch
import torch.nn.functional as F

from oracle import tactilesr_oracle as O


def oracle_grads(sd, LR, HR, scale_factor=10, dtype=torch.float64, masks=None, record=False):
    """loss, {param: grad}, new BN stats and (optionally) the ReLU pre-activations of one train-mode forward +
    backward of the CPU oracle in `dtype`, with the ReLU pattern optionally forced to `masks`."""
    leaves = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items() if O.is_trainable(k)}
    full = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    full.update(leaves)
    tap = O.ReluTap(masks=masks, record=record) if (masks is not None or record) else None
    ns = {}
    out = O.tactilesr_forward(full, LR.to(dtype), scale_factor=scale_factor, training=True, new_stats=ns, tap=tap)
    loss = F.mse_loss(out, HR.to(dtype))
    gl = torch.autograd.grad(loss, list(leaves.values()))
    return float(loss), dict(zip(leaves, gl)), ns, (tap.pre if tap is not None else None)


def check_pattern(hip_masks, pre64, flip_tol=1e-5, max_flip_frac=2e-5):
    """HIP activation pattern vs the fp64 oracle's: every disagreement must sit at a pre-activation that is zero to
    rounding.  Returns the number of flipped elements."""
    assert set(hip_masks) == set(pre64), (sorted(set(hip_masks) ^ set(pre64)))
    flips = total = 0
    for name, pre in pre64.items():
        hm = hip_masks[name].cpu()
        assert hm.shape == pre.shape, (name, hm.shape, pre.shape)
        diff = hm != (pre > 0)
        n = int(diff.sum())
        total += pre.numel()
        if n:
            worst = float(pre[diff].abs().max() / pre.abs().max())
            assert worst < flip_tol, f"{name}: mask differs where the fp64 pre-activation is {worst:.2e} of max"
            flips += n
    assert flips <= max(4, max_flip_frac * total), (flips, total)
    return flips


def check_grads(named_grads, g64m, tol=2e-5, zero_tol=1e-4):
    """max-norm bar on EVERY parameter gradient against the fp64 gradient evaluated on the HIP masks."""
    worst = (0.0, None)
    bad = []
    for k, ref in g64m.items():
        got = named_grads[k].detach().cpu().double()
        den = float(ref.abs().max())
        if den < 1e-6:            # conv bias in front of a train-mode BN: the exact gradient is 0
            assert float(got.abs().max()) < zero_tol, k
            continue
        e = float((got - ref).abs().max()) / den
        if e > worst[0]:
            worst = (e, k)
        if not e <= tol:
            bad.append((k, e))
    assert not bad, bad
    return worst


# ------------------------------------------------------------------------------ whole-step checks shared by GPU tests
def relerr(a, b):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def step_data(cfg, B, seed):
    """Seeded state dict (the oracle's random law) and one batch (LR taxels, HR target at 4sf x 4sf) for `cfg`."""
    sf, Tn = cfg.get("scale_factor", 10), cfg.get("seqsCnt", 1)
    sd = O.random_state_dict(O.tactilesr_state_shapes(**cfg), seed)
    g = torch.Generator().manual_seed(seed + 1)
    LR = torch.rand(B, 3 * Tn, 4, 4, generator=g) * 8
    HR = torch.rand(B, 1, 4 * sf, 4 * sf, generator=g) * 25
    return sd, LR, HR


def train_step_vs_oracle(T, cfg, B, seed, tol=1e-5, loss_tol=1e-5, impl=None, record=None):
    """One train-mode forward + backward of the HIP model against the fp64 oracle: loss within `loss_tol`, running
    statistics within 1e-5, the ReLU pattern equal to fp64's up to rounding-zero flips, every parameter gradient within
    `tol` (max-norm) of the fp64 gradient on the device's pattern.  `record`, when given, is the cached
    `oracle_grads(.., record=True)` result of the same (sd, LR, HR).  Returns (model, worst gradient error)."""
    sf = cfg.get("scale_factor", 10)
    sd, LR, HR = step_data(cfg, B, seed)
    l64, _, ns64, pre64 = record if record is not None else oracle_grads(sd, LR, HR, scale_factor=sf, record=True)
    m = T.TactileSR(**cfg)
    if impl is not None:
        m.train_impl = impl
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train()
    eng = m.train_engine()
    eng.keep_ctx = True              # forward keeps its context: the test reads the activation pattern back
    out = m(LR.cuda())
    loss = F.mse_loss(out, HR.cuda())
    assert abs(loss.item() - l64) < loss_tol * abs(l64)
    loss.backward()
    new_sd = m.state_dict()
    for k, v in ns64.items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            assert relerr(new_sd[k], v) < 1e-5, k
    masks = {k: v.cpu() for k, v in eng.activation_masks(eng.last_ctx).items()}
    flips = check_pattern(masks, pre64)
    _, g64m, _, _ = oracle_grads(sd, LR, HR, scale_factor=sf, masks=masks)
    worst = check_grads({k: p.grad for k, p in m.named_parameters()}, g64m, tol=tol)
    print(f"[train-vs-oracle {cfg} B={B}{' ' + impl if impl else ''}] {flips} ReLU flips; worst on-pattern grad error "
          f"{worst[0]:.2e} ({worst[1]})")
    return m, worst


def emulated_step(sd, LR, HR, **kw):
    """Loss, gradients and new running statistics of the oracle's bf16-emulating train forward (`emulate="bf16"`)."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items() if O.is_trainable(k)}
    full = dict(sd)
    full.update(leaves)
    ns = {}
    out = O.tactilesr_forward(full, LR, training=True, new_stats=ns, emulate="bf16", **kw)
    loss = F.mse_loss(out, HR)
    gl = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
    grads = {k: (g if g is not None else torch.zeros_like(leaves[k])) for k, g in zip(leaves, gl)}
    return float(loss), grads, ns, out.detach()


def bf16_train_step_vs_emulating_oracle(T, cfg, B, seed):
    """train_impl = "bf16" (bf16 CB16 storage of every activation / gradient tensor) against the oracle's emulation of that
    arithmetic: loss within 2e-3, output max-norm within 2^-6, running statistics within 2e-3, every parameter gradient
    at cosine >= 0.995 and norm ratio within 5 % of the emulated one (bars and reasons:
    test_gpu_train.test_train_step_bf16_storage_vs_bf16_emulating_oracle)."""
    sf = cfg.get("scale_factor", 10)
    sd, LR, HR = step_data(cfg, B, seed)
    l_e, g_e, ns_e, out_e = emulated_step(sd, LR, HR, scale_factor=sf)
    m = T.TactileSR(**cfg)
    m.train_impl = "bf16"            # explicit arithmetic choice (no environment switch)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train()
    eng = m.train_engine()
    eng.keep_ctx = True
    assert eng.io16 and eng.act_dtype == torch.bfloat16
    out = m(LR.cuda())
    ctx = eng.last_ctx
    assert all(t.dtype == torch.bfloat16 for t in (ctx.hcat, ctx.h0, ctx.zf, ctx.catT, ctx.blocks[0].cat1, ctx.blocks[0].cat2))
    loss = F.mse_loss(out, HR.cuda())
    e_out = relerr(out, out_e)
    assert e_out <= 2.0 ** -6 and abs(loss.item() - l_e) <= 2e-3 * abs(l_e), (e_out, loss.item(), l_e)
    loss.backward()
    new_sd = m.state_dict()
    for k, v in ns_e.items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            assert relerr(new_sd[k], v) < 2e-3, k
    worst = 1.0
    for k, p in m.named_parameters():
        ref = g_e[k].double().flatten()
        got = p.grad.detach().cpu().double().flatten()
        if float(ref.abs().max()) < 1e-6 * float(max(v.abs().max() for v in g_e.values())):
            continue                                    # conv bias in front of a train-mode BN: gradient == 0 + noise
        cos = float(got @ ref / (got.norm() * ref.norm()).clamp_min(1e-30))
        worst = min(worst, cos)
        assert cos >= 0.995, (k, cos)
        assert abs(float(got.norm() / ref.norm()) - 1.0) < 5e-2, (k, float(got.norm() / ref.norm()))
    print(f"[bf16-storage train vs bf16 oracle {cfg} B={B}] out {e_out:.2e}, loss {abs(loss.item() - l_e) / abs(l_e):.2e}, "
          f"worst gradient cosine {worst:.5f}")
    return m


def bf16_ulp(ref):
    """Spacing of bf16 at |ref| (8 significand bits): 2^(floor(log2|ref|) - 7); the smallest normal spacing for 0."""
    a = ref.abs().double().clamp_min(2.0 ** -126)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - 7)


def bf16_eval_vs_emulating_oracle(T, cfg, sd, LR, exempt_e2e_out=False):
    """conv_impl = "bf16" eval forward against the oracle's emulation of its arithmetic: (1) teacher-forced per stage (the
    parity check) and (2) end to end at the stated 3e-2 (reasons: test_gpu_parity.
    test_model_eval_forward_bf16_storage_vs_bf16_emulating_oracle).  `exempt_e2e_out` leaves the final image out of (2).
    Returns (worst differing share, worst beyond-one-ulp share, worst max-norm, worst rel-L2, e2e rel-L2, e2e max, output)."""
    sf = cfg.get("scale_factor", 10)
    m = T.TactileSR(**cfg)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    m.conv_impl = "bf16"
    y, stages = m.forward_with_stages(LR.cuda())
    y = y.cpu()
    dev = {k: v.cpu() for k, v in stages.items()}
    assert all(torch.equal(v, v.to(torch.bfloat16).float()) for v in dev.values())
    forced, free = {}, {}
    with torch.no_grad():
        yf = O.tactilesr_forward(sd, LR, sf, stages=forced, emulate="bf16", teacher=dev)
        ye = O.tactilesr_forward(sd, LR, sf, stages=free, emulate="bf16")
        # The oracle has no teacher point between ResBlocks, so with several of them its "force" would answer "force_in"
        # across all of them, and a rounding-boundary flip in one block would cascade into the comparison of the next
        # (each conv multiplies the differing share ~10x).  Restate the branch block by block on the device's own
        # intermediates ("res{i}" of forward_with_stages): every block, the last one ("force") included, is then the
        # oracle's answer to the DEVICE's input, under the same per-stage bars.  One ResBlock: nothing changes.
        n_res = O._count(sd, "forceFeatureExtra_layer")
        for i in range(n_res if n_res > 1 else 0):
            x_in = dev["force_in"] if i == 0 else dev[f"res{i - 1}"]
            forced["force" if i == n_res - 1 else f"res{i}"] = O.resblock_forward(sd, f"forceFeatureExtra_layer.{i}", x_in,
                                                                                 emulate="bf16")
    w_same = w_ulp = w_max = w_l2 = 0.0
    for name, ref in list(forced.items()) + [("out", yf)]:
        got = (y if name == "out" else dev[name]).double()
        d = (got - ref.double()).abs()
        mx = float(ref.abs().max())
        if name == "out":      # fp32 head output on the device's head0: no rounding, only accumulation-order noise
            assert float(d.max()) <= 1e-5 * mx, name
            continue
        differ = float((d > 0).double().mean())
        beyond = float((d > bf16_ulp(ref) * 1.001 + 2e-4 * mx).double().mean())
        l2 = float(d.norm() / ref.double().norm())
        w_same, w_ulp, w_max, w_l2 = max(w_same, differ), max(w_ulp, beyond), max(w_max, float(d.max()) / mx), max(w_l2, l2)
        assert differ < 1e-2 and beyond < 1e-3 and float(d.max()) <= 1e-2 * mx and l2 <= 1e-3, (name, differ, beyond, float(d.max()) / mx, l2)
    e2e_l2 = e2e_max = 0.0
    for name, ref in list(free.items()) + [("out", ye)]:
        got = (y if name == "out" else dev[name]).double()
        l2 = float((got - ref.double()).norm() / ref.double().norm())
        mx = float((got - ref.double()).abs().max() / ref.abs().max())
        e2e_l2, e2e_max = max(e2e_l2, l2), max(e2e_max, mx)
        assert (exempt_e2e_out and name == "out") or (l2 <= 3e-2 and mx <= 5e-2), (name, l2, mx)
    return w_same, w_ulp, w_max, w_l2, e2e_l2, e2e_max, y
