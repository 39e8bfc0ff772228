"""Shared by tests/test_adam_ex_cpu.py and tests/test_gpu_adam_ex.py: the case tables (with the reason for every case),
the restatement of the extended Adam launch (include/tactilesr_hip.h, tsr_adam_multi_ex) in fp64 and, operation by
operation, in fp32, the comparison rule with its checker, and the guarded launch harness.

The rule is the one the legacy launch is held to (tests/test_gpu_train.py, the fused multi-tensor Adam test): per tensor,
``relerr(hip, fp64) <= max(1e-6, 4 * relerr(fp32 yardstick, fp64))`` with ``relerr = max|a - b| / max|b|``.  The step
m / (sqrt(v) / bc2_sqrt + eps) is ill-conditioned where the gradient cancels to about eps, so an honest fp32 evaluation
of the same formula is itself off fp64 by more than a few ulps there; the yardstick term measures exactly that, on the
same data, and the factor 4 covers another legitimate association of the same fp32 operations (fused multiply-adds).
The yardstick is torch's own fp32 CPU optimizer where torch is the reference, and the restatement below evaluated in
fp32 with numpy (every operation rounded on its own) where the restatement is.  The moments have no such cancellation:
they are held to 1e-6 of the yardstick's (three fp32 roundings of 2^-24 each, relative to the tensor's maximum).
"""
import ctypes

import numpy as np
import torch

DECOUPLED, AMSGRAD = 1, 2
# the three flag combinations the extended launch adds (flags = 0 is torch.optim.Adam's formula, the legacy launch's)
FLAG_CASES = ((DECOUPLED, "adamw"), (AMSGRAD, "adam_amsgrad"), (DECOUPLED | AMSGRAD, "adamw_amsgrad"))
FLAG_IDS = [name for _, name in FLAG_CASES]
ALL_FLAGS = (0,) + tuple(f for f, _ in FLAG_CASES)

# tensor sizes (elements): 1, 3 the scalar tail alone; 4 the first 16-byte access; 5 one access and a tail word; 255 /
# 256 / 257 round the workgroup's 256 threads on the scalar path (64 / 64.25 vector lanes on the other); 1023..1025
# four vector passes of the first lanes and one word more; 4095 / 4096 / 4097 the last short chunk, an exactly full
# chunk, and a full chunk followed by a one-element chunk; 2 * 4096 + 7 two full chunks and a 7-word tail (one vector
# access and three scalar words).
SIZES = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 2 * 4096 + 7)

POINTERS = ("param", "grad", "exp_avg", "exp_avg_sq", "vmax")


def offset_cases(flags):
    """(id, {pointer: floats off 16-byte alignment}): everything aligned (the vector path), each pointer alone 1, 2 and 3
    floats off (ONE misaligned pointer must send the whole record down the scalar path -- vmax too, which the record
    itself does not hold), and all of them off together.  vmax only exists with AMSGRAD."""
    names = [n for n in POINTERS if n != "vmax" or flags & AMSGRAD]
    out = [("aligned", {})]
    for off in (1, 2, 3):
        out += [(f"{n}+{off}", {n: off}) for n in names]
        out.append((f"all+{off}", {n: off for n in names}))
    return out


# the boundary sweep's scalars: 1 - lr * wd = 0.999 is clearly below 1, so a lost or doubled decay shows
B_LR, B_WD, B_BETAS, B_EPS = 1e-2, 0.1, (0.9, 0.999), 1e-8


def f32(x) -> float:
    """x rounded to float, as a Python double: what a `float` argument of the C ABI receives."""
    return float(np.float32(x))


def hyper(lr, beta1, beta2, step, weight_decay, flags):
    """{lr, bc1, bc2_sqrt, decay} as tsr_adam_hyper_ex defines them: formed in double from the float lr and weight_decay
    the call receives, rounded to float once."""
    lr, wd = f32(lr), f32(weight_decay)
    decay = np.float32(1.0 - lr * wd) if flags & DECOUPLED else np.float32(1.0)
    return (np.float32(lr), np.float32(1.0 - beta1 ** step), np.float32(np.sqrt(1.0 - beta2 ** step)), decay)


def restate(p, g, m, v, vm, lr, betas, eps, weight_decay, step, flags, coef=None, dtype=np.float64):
    """One step of the extended launch on numpy arrays, returning (p, g, m, v, vm) after it (g is the clipped gradient
    the launch leaves in place; vm is None without AMSGRAD).

    dtype=float64 is the restatement: the formulas of the header in double with the scalars as given.  dtype=float32
    is the yardstick: the scalars rounded as the launch rounds them ({lr, bc1, bc2_sqrt, decay} through ``hyper``, the
    betas and 1 - beta formed in double and rounded) and every operation rounded to fp32 on its own (numpy does not
    fuse)."""
    b1, b2 = betas
    T = dtype
    if T == np.float32:
        lr_, bc1, bc2s, decay = hyper(lr, b1, b2, step, weight_decay, flags)
        b1_, b2_, o1, o2 = T(b1), T(b2), T(1.0 - b1), T(1.0 - b2)
        eps_, wd_ = T(eps), T(weight_decay)
    else:
        lr_, bc1, bc2s = lr, 1.0 - b1 ** step, np.sqrt(1.0 - b2 ** step)
        decay = 1.0 - lr * weight_decay if flags & DECOUPLED else 1.0
        b1_, b2_, o1, o2, eps_, wd_ = b1, b2, 1.0 - b1, 1.0 - b2, eps, weight_decay
    with np.errstate(all="ignore"):
        w, g, m, v = (np.asarray(a, dtype=T) for a in (p, g, m, v))
        if coef is not None:
            g = g * T(coef)
        if flags & DECOUPLED:
            gg, w0 = g, w * T(decay)
        else:
            gg, w0 = wd_ * w + g, w
        m = b1_ * m + o1 * gg
        v = b2_ * v + o2 * gg * gg
        if flags & AMSGRAD:
            vm = np.maximum(np.asarray(vm, dtype=T), v)          # numpy's maximum propagates a NaN, like torch's
            vhat = vm
        else:
            vm, vhat = None, v
        p = w0 - (T(lr_) / T(bc1)) * (m / (np.sqrt(vhat) / T(bc2s) + eps_))
    return p, g, m, v, vm


def relerr(a, b) -> float:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def check_param(got, yard32, ref64, label=""):
    """The rule: relerr(got, fp64) <= max(1e-6, 4 * relerr(fp32 yardstick, fp64)).  Returns (error, bar)."""
    e_got, e_yard = relerr(got, ref64), relerr(yard32, ref64)
    bar = max(1e-6, 4 * e_yard)
    assert e_got <= bar, f"{label}: parameter {e_got:.3e} off fp64, bar {bar:.3e} (yardstick {e_yard:.3e})"
    return e_got, bar


def check_moment(got, yard32, label=""):
    e = relerr(got, yard32)
    assert e <= 1e-6, f"{label}: {e:.3e} off the fp32 yardstick, bar 1e-6"
    return e


def check_step(got, before, scalars, step, flags, coef=None, label=""):
    """``got`` / ``before``: dicts of fp32 numpy arrays (param, grad, exp_avg, exp_avg_sq[, vmax]) after / before one
    launch with scalars = (lr, betas, eps, weight_decay).  Asserts the rule for the parameter and 1e-6 for the moments
    and the clipped gradient.  Returns the parameter's (error, bar)."""
    lr, betas, eps, wd = scalars
    args = (before["param"], before["grad"], before["exp_avg"], before["exp_avg_sq"], before.get("vmax"))
    r64 = restate(*args, f32(lr), betas, f32(eps), f32(wd), step, flags, coef)
    r32 = restate(*args, lr, betas, eps, wd, step, flags, coef, dtype=np.float32)
    out = check_param(got["param"], r32[0], r64[0], label)
    check_moment(got["exp_avg"], r32[2], f"{label} exp_avg")
    check_moment(got["exp_avg_sq"], r32[3], f"{label} exp_avg_sq")
    if flags & AMSGRAD:
        check_moment(got["vmax"], r32[4], f"{label} max_exp_avg_sq")
    # the gradient: one fp32 multiply (nothing at all without clipping), so the yardstick's bits
    assert np.array_equal(got["grad"].view(np.int32), np.asarray(r32[1], dtype=np.float32).view(np.int32)), f"{label}: grad"
    return out


def state_case(n, seed, step=3):
    """(p, g, m, v, vm) fp32 numpy vectors of a state as a few steps leave it: sqrt(v) well above |m| / 50 so the update
    stays of the order of lr, vm partly above and partly below the v the step will produce (both sides of the maximum)."""
    r = np.random.default_rng(seed)
    p = r.standard_normal(n).astype(np.float32)
    g = (r.standard_normal(n) * 1e-2).astype(np.float32)
    if step == 1:
        z = np.zeros(n, np.float32)
        return p, g, z, z.copy(), z.copy()
    m = (r.standard_normal(n) * 1e-2).astype(np.float32)
    v = (r.random(n) * 1e-2 + 1e-3).astype(np.float32)
    vm = (v * np.where(r.random(n) < 0.5, 0.5, 2.0)).astype(np.float32)
    return p, g, m, v, vm


def bits(t):
    """The raw 4-byte words of a tensor or array, as a flat int32 CPU tensor."""
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t))
    return t.detach().cpu().contiguous().view(-1).view(torch.int32).clone()


# ------------------------------------------------------------------------------------------ the guarded launch harness
SENTINEL = 0x7FC0BEEF      # a quiet NaN with a payload, as int32
GUARD = 8                  # guard words around every tensor


class Rec(ctypes.Structure):           # tsr_adam_chunk, declared here too so that the layout itself is under test
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p),
                ("exp_avg_sq", ctypes.c_void_p), ("n", ctypes.c_int), ("reserved", ctypes.c_int)]


class Guarded:
    """Five device buffers (param, grad, exp_avg, exp_avg_sq, vmax), each prefilled with a NaN sentinel and holding
    every tensor of ``tensors`` (a list of dicts name -> fp32 array) ``offsets[name]`` words past a 16-byte boundary
    with >= GUARD sentinel words on both sides.  ``override`` = {tensor index: (n,)}: that tensor gets ONE record with
    this n instead of its chunks (a deliberately bad record)."""

    def __init__(self, tensors, flags, offsets=None, override=None):
        offsets = offsets or {}
        self.names = [n for n in POINTERS if n != "vmax" or flags & AMSGRAD]
        self.n = [int(t["param"].size) for t in tensors]
        self.sides = {}
        for name in self.names:
            off = offsets.get(name, 0)
            pos, starts = GUARD, []
            for n in self.n:
                pos = -(-pos // 4) * 4 + off
                starts.append(pos)
                pos += n + GUARD
            host = torch.full((pos + GUARD,), SENTINEL, dtype=torch.int32)
            inside = torch.zeros(pos + GUARD, dtype=torch.bool)
            for t, st, n in zip(tensors, starts, self.n):
                inside[st:st + n] = True
                host[st:st + n] = bits(t[name])
            self.sides[name] = (host, inside, starts)
        self.dev = {name: self.sides[name][0].cuda() for name in self.names}
        for name in self.names:
            assert self.dev[name].data_ptr() % 16 == 0
        recs, vptr = [], []
        for i, n in enumerate(self.n):
            base = {name: self.dev[name].data_ptr() + 4 * self.sides[name][2][i] for name in self.names}
            pieces = [(0, override[i][0])] if override is not None and i in override else \
                [(o, min(4096, n - o)) for o in range(0, n, 4096)]
            for o, cn in pieces:
                recs.append(tuple(base[k] + 4 * o for k in POINTERS[:4]) + (cn, 0))
                if flags & AMSGRAD:
                    vptr.append(base["vmax"] + 4 * o)
        arr = (Rec * len(recs))(*recs)
        self.table = torch.frombuffer(memoryview(arr).cast("B"), dtype=torch.uint8).clone().cuda()
        self.vtable = None
        if flags & AMSGRAD:
            varr = (ctypes.c_void_p * len(vptr))(*vptr)
            self.vtable = torch.frombuffer(memoryview(varr).cast("B"), dtype=torch.uint8).clone().cuda()
        self.n_chunks = len(recs)

    def read(self):
        """[{name: fp32 array}] per tensor, after asserting that every guard word is still the sentinel."""
        out = [dict() for _ in self.n]
        for name in self.names:
            host, inside, starts = self.sides[name]
            now = self.dev[name].cpu()
            assert bool((now[~inside] == SENTINEL).all()), f"a guard word of {name} was written"
            for o, st, n in zip(out, starts, self.n):
                o[name] = now[st:st + n].clone().view(torch.float32).numpy()
        return out


def launch(tensors, flags, scalars, step, offsets=None, override=None, dev_form=False, coef=None, hyper4=None):
    """One tsr_adam_multi_ex (``dev_form``: tsr_adam_multi_ex_dev, reading ``hyper4`` or the floats of ``hyper``) launch
    over the guarded layout, run twice from the same bits: both runs must agree bit for bit.  scalars = (lr, betas, eps,
    weight_decay); ``coef`` (None: no clipping) goes through a device float.  Returns [{name: fp32 array}] after it."""
    from tactilesr_amd import _lib
    lr, (b1, b2), eps, wd = scalars
    F, I, D = ctypes.c_float, ctypes.c_int, ctypes.c_double
    results = []
    for _ in range(2):
        g = Guarded(tensors, flags, offsets, override)
        clip = torch.tensor([coef], dtype=torch.float32).cuda() if coef is not None else None
        head = (_lib.ptr(g.table), _lib.ptr(g.vtable), I(g.n_chunks), I(flags))
        if dev_form:
            h = hyper4 if hyper4 is not None else hyper(lr, b1, b2, step, wd, flags)
            hd = torch.tensor([float(x) for x in h], dtype=torch.float32).cuda()
            _lib.call("tsr_adam_multi_ex_dev", *head, _lib.ptr(hd), D(b1), D(b2), F(eps), F(wd), _lib.ptr(clip), _lib.stream())
        else:
            _lib.call("tsr_adam_multi_ex", *head, F(lr), D(b1), D(b2), F(eps), F(wd), I(step), _lib.ptr(clip), _lib.stream())
        torch.cuda.synchronize()
        results.append(g.read())
    for x, y in zip(*results):
        for k in x:
            assert np.array_equal(x[k].view(np.int32), y[k].view(np.int32)), f"two runs from the same bits differ in {k}"
    return results[0]


def same_bits(a, b) -> bool:
    return a.shape == b.shape and np.array_equal(np.asarray(a, np.float32).view(np.int32), np.asarray(b, np.float32).view(np.int32))
