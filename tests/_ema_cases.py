"""Shared by tests/test_ema_cpu.py and tests/test_gpu_ema.py: the case tables (with the reason for every case), the
fp64 restatement of the averaging update, the derived error bound with its checker, and the guarded launch harness.

The bound is derived, not measured.  The kernel computes ``fmaf(omd, src - avg, avg)`` with the subtraction rounded in
fp32: that subtraction errs by at most 2^-24 |src - avg| <= 2^-23 max(|src|, |avg|), the factor omd <= 1 does not
enlarge it, and the fma rounds once, at most 2^-24 |result| <= 2^-24 max(|src|, |avg|).  Hence, per element,
|kernel - fp64| <= 3 * 2^-24 * max(|src|, |avg|).  (The cases keep results in the normal range: a subnormal result is
rounded to an absolute 2^-150, which no relative bound covers.)  The restatement takes ``omd`` as the fp32 value the launch
is handed, so the rounding of 1 - decay is not part of the error.
"""
import ctypes

import torch

BOUND = 3 * 2.0 ** -24
UPDATE, STORE, LOAD, SWAP = 0, 1, 2, 3

# tensor sizes (elements) of the size sweep: 1..5 the scalar tail alone and the first 16-byte access; 255 / 256 / 257
# round the workgroup's 256 threads (one pass of scalar lanes, 64 / 64.25 vector lanes); 1023..1025 four vector passes
# and one word more; 4095 / 4096 / 4097 the last short chunk, an exactly full chunk, and a full chunk followed by a
# single-element chunk; 8191 / 8193 two chunks, the second one word short / a third of one word; 3 * 4096 + 7 three
# full chunks and a 7-word tail (a vector access and three scalar words).
SIZES = (1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8193, 3 * 4096 + 7)

# one_minus_decay: 1 (SWA's first update: the average becomes src), 0.5 (both operands weigh), 1e-3 and 1e-4 (decay 0.999
# and 0.9999: the increment is far below the average), 0 (the average must not move).
OMDS = (1.0, 0.5, 1e-3, 1e-4, 0.0)


def _g(seed):
    return torch.Generator().manual_seed(seed)


def value_cases(n=4099):
    """name -> (avg, src) fp32 vectors, with the reason for every case."""
    r = lambda s: torch.randn(n, generator=_g(s))
    a = r(1)
    scale = 10.0 ** torch.randint(-20, 21, (n,), generator=_g(7)).float()
    return {
        "normal": (a, r(2)),                                     # unrelated operands of one magnitude
        "close": (a, a * (1 + 1e-3 * r(3))),                     # the training regime: src - avg cancels (exact by Sterbenz)
        "equal": (a, a.clone()),                                 # a frozen parameter: the average must not move at all
        "zero_avg": (torch.zeros(n), r(4)),                      # a fresh zero shadow; omd == 1 must give src exactly
        "opposite": (a, -a),                                     # |src - avg| = 2 max: the subtraction term's worst case
        "scales": (a * scale, r(5) * scale),                     # the bound is per element: 41 decades in one tensor
        "lost_increment": (a.abs() + 1e10, r(6) * 1e-10),        # the increment is far below half an ulp of the average
    }


def omd32(omd) -> float:
    """The fp32 value a launch is handed for the Python double ``omd``."""
    return float(torch.tensor(float(omd), dtype=torch.float32))


def restatement(avg, src, omd):
    """The update in fp64: avg + omd * (src - avg), ``omd`` rounded to fp32 first as the launch takes it."""
    a, s = avg.double(), src.double()
    return a + omd32(omd) * (s - a)


def fp32_eval(avg, src, omd):
    """The kernel's arithmetic restated on the host: the subtraction rounded in fp32, the multiply-add formed exactly in
    fp64 (a 24 x 24-bit product plus an fp32 value) and rounded to fp32."""
    d = (src.float() - avg.float())
    return (omd32(omd) * d.double() + avg.double()).float()


def check(got, avg, src, omd, label=""):
    """Assert |got - restatement| <= BOUND * max(|src|, |avg|) per element; where the restatement is not finite the
    result is not finite in the same way.  Returns the worst error as a fraction of the bound."""
    want = restatement(avg, src, omd)
    assert got.dtype == torch.float32 and got.shape == want.shape, (label, got.dtype, got.shape)
    finite = torch.isfinite(want)
    assert torch.equal(torch.isnan(got), torch.isnan(want)), f"{label}: NaN pattern differs"
    inf = torch.isinf(want)
    assert torch.equal(got[inf].double(), want[inf]), f"{label}: Inf pattern differs"
    lim = BOUND * torch.maximum(avg.double().abs(), src.double().abs())[finite]
    err = (got.double()[finite] - want[finite]).abs()
    bad = err > lim
    assert not bool(bad.any()), (f"{label}: {int(bad.sum())} elements outside 3 * 2^-24 * max(|src|, |avg|); worst "
                                 f"{float((err / lim.clamp_min(1e-300)).max()):.3f} of the bound")
    return float((err / lim.clamp_min(1e-300)).max()) if err.numel() else 0.0


def bits(t):
    """The raw 4-byte words of a tensor, as a flat int32 CPU tensor (int64 as two words per element)."""
    return t.detach().cpu().contiguous().view(-1).view(torch.int32).clone()


# ------------------------------------------------------------------------------------------ the guarded launch harness
SENTINEL = 0x7FC0BEEF      # a quiet NaN with a payload, as int32
GUARD = 8                  # guard words around every tensor


class Rec(ctypes.Structure):           # tsr_ema_chunk, declared here too so that the layout itself is under test
    _fields_ = [("avg", ctypes.c_void_p), ("src", ctypes.c_void_p), ("n", ctypes.c_int), ("mode", ctypes.c_int)]


class Guarded:
    """Tensors of raw words laid out in two device buffers (the averages, the sources) that are prefilled with a NaN
    sentinel: every tensor starts ``off`` words past a 16-byte boundary and has >= GUARD sentinel words on both sides.
    ``avg`` entries may be ``None``: that shadow keeps the NaN prefill (what STORE has to overwrite)."""

    def __init__(self, avg, src, modes, avg_off=0, src_off=0, override=None):
        self.n = [int(bits(s).numel()) for s in src]          # in 4-byte words
        self.modes = list(modes)
        self.sides = []
        for data, off in ((avg, avg_off), (src, src_off)):
            pos, starts = GUARD, []
            for n in self.n:
                pos = -(-pos // 4) * 4 + off
                starts.append(pos)
                pos += n + GUARD
            host = torch.full((pos + GUARD,), SENTINEL, dtype=torch.int32)
            inside = torch.zeros(pos + GUARD, dtype=torch.bool)
            for d, st, n in zip(data, starts, self.n):
                inside[st:st + n] = True
                if d is not None:
                    host[st:st + n] = bits(d)
            self.sides.append((host, inside, starts))
        self.dev = [side[0].cuda() for side in self.sides]
        recs = []
        for i, n in enumerate(self.n):
            pa = self.dev[0].data_ptr() + 4 * self.sides[0][2][i]
            ps = self.dev[1].data_ptr() + 4 * self.sides[1][2][i]
            if override is not None and i in override:          # a deliberately bad record, one per tensor
                recs.append((pa, ps) + tuple(override[i]))
                continue
            for o in range(0, n, 4096):
                recs.append((pa + 4 * o, ps + 4 * o, min(4096, n - o), self.modes[i]))
        arr = (Rec * len(recs))(*recs)
        self.table = torch.frombuffer(memoryview(arr).cast("B"), dtype=torch.uint8).clone().cuda()
        self.n_chunks = len(recs)

    def read(self):
        """([avg words], [src words]) as int32 CPU tensors, after asserting that every guard word is still the sentinel."""
        out = []
        for (host, inside, starts), dev in zip(self.sides, self.dev):
            now = dev.cpu()
            assert bool((now[~inside] == SENTINEL).all()), "a guard word was written"
            out.append([now[st:st + n].clone() for st, n in zip(starts, self.n)])
        return out


def launch(avg, src, modes, op, omd, avg_off=0, src_off=0, override=None, dev_form=False, repeat=1):
    """One launch (``repeat`` launches in a row) over the guarded layout, run twice from the same bits: both runs must
    agree bit for bit.  Returns ([avg words], [src words]) after the launch."""
    from tactilesr_amd import _lib
    results = []
    for _ in range(2):
        g = Guarded(avg, src, modes, avg_off, src_off, override)
        scalar = torch.tensor([omd], dtype=torch.float32).cuda() if dev_form else None
        for _ in range(repeat):
            if dev_form:
                _lib.call("tsr_ema_multi_dev", _lib.ptr(g.table), ctypes.c_int(g.n_chunks), ctypes.c_int(op),
                          _lib.ptr(scalar), _lib.stream())
            else:
                _lib.call("tsr_ema_multi", _lib.ptr(g.table), ctypes.c_int(g.n_chunks), ctypes.c_int(op),
                          ctypes.c_float(omd), _lib.stream())
        torch.cuda.synchronize()
        results.append(g.read())
    for x, y in zip(results[0][0] + results[0][1], results[1][0] + results[1][1]):
        assert torch.equal(x, y), "two runs from the same bits differ"
    return results[0]


def as_f32(words):
    return words.view(torch.float32)
