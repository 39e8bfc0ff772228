"""Poisoned workspaces (tests/test_poison_cpu.py, tests/test_gpu_workspace_poison.py, tests/test_gpu_call_history.py).

The library allocates no device memory of its own: every workspace a kernel sees comes from `torch.empty`,
`torch.empty_like` or `Tensor.new_empty`, and the caching allocator hands back the block the previous identical call just
used.  A kernel that reads a region this call never wrote therefore finds last call's correct values there, and every test
that runs a fresh object once passes.  `poisoned(byte)` replaces the three allocation names for its duration and fills the
storage of every floating-point tensor they return with `byte`:

    byte   fp32      bf16      fp16    fp64      purpose
    0xFF   NaN       NaN       NaN     NaN       propagating poison
    0x7B   1.3e36    1.3e36    61280   6.5e286   finite in all four types: fmaxf and the max|x| atomics drop a NaN, a stale
                                                 huge max|x| slot or amax operand survives

Integer and bool tensors come back untouched: a poisoned index would be an out-of-bounds address.  The fill goes through the
ordinary stream (`Tensor.fill_`), so inside a graph capture it is captured and every replay poisons again.
"""
import contextlib

import torch

NAN_BYTE = 0xFF
HUGE_BYTE = 0x7B
BYTES = (NAN_BYTE, HUGE_BYTE)
# what one element of each type reads as after the fill (NaN for 0xFF); tests/test_poison_cpu.py holds the fill to these
HUGE_VALUE = {torch.float32: 1.3057709929374801e36, torch.bfloat16: 1.3032665114922417e36, torch.float16: 61280.0,
              torch.float64: 6.538675761325367e286}

_raw_empty = getattr(torch.empty, "__wrapped__", torch.empty)
_NAMES = ((torch, "empty"), (torch, "empty_like"), (torch.Tensor, "new_empty"))


def fill_storage(t, byte):
    """Fill the whole storage behind the floating-point tensor `t` with `byte`; anything else is left alone."""
    if not isinstance(t, torch.Tensor) or not t.is_floating_point() or t.device.type == "meta":
        return t
    st = t.untyped_storage()
    if st.nbytes() == 0:
        return t
    with torch.no_grad():
        _raw_empty(0, dtype=torch.uint8, device=t.device).set_(st).fill_(byte)
    return t


def _wrap(orig, byte, counter):
    def alloc(*args, **kwargs):
        t = orig(*args, **kwargs)
        if kwargs.get("out") is None:         # (`out=` resizes a tensor of the caller's: not a fresh workspace)
            fill_storage(t, byte)
            counter[0] += 1
        return t
    alloc.__wrapped__ = orig
    return alloc


@contextlib.contextmanager
def poisoned(byte):
    """Replace `torch.empty`, `torch.empty_like` and `torch.Tensor.new_empty` by versions that fill what they return with
    `byte`; the three names are restored on exit, also after an exception.  Nests: the inner fill is the one that stays.
    Yields a one-element list counting the allocations that went through the replaced names."""
    assert 0 <= int(byte) <= 0xFF
    saved = [(owner, name, getattr(owner, name)) for owner, name in _NAMES]
    counter = [0]
    try:
        for owner, name, orig in saved:
            setattr(owner, name, _wrap(orig, int(byte), counter))
        yield counter
    finally:
        for owner, name, orig in saved:
            setattr(owner, name, orig)


@contextlib.contextmanager
def plain():
    """The do-nothing twin of `poisoned`, so that a test runs `with ctx():` over (plain, poisoned(0xFF), poisoned(0x7B))."""
    yield [0]


def runs():
    """The three runs of every poison case: (label, context-manager factory)."""
    return (("plain", plain), ("0xFF", lambda: poisoned(NAN_BYTE)), ("0x7B", lambda: poisoned(HUGE_BYTE)))
