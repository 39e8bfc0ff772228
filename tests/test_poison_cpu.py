"""tests/_poison.py without a GPU: the two fill patterns in every floating type, integers and bools left alone, restoration
(also after an exception), nesting, and that `tactilesr_amd` reaches `torch.empty`, `torch.empty_like` and
`Tensor.new_empty` through the attributes the manager replaces (its CPU-side helpers that allocate come back filled)."""
import struct
import types

import pytest
import torch

import _poison as P
from tactilesr_amd import ddp
from tactilesr_amd import functional as F
from tactilesr_amd.model import tactileSR_model as TM

FLOATS = (torch.float32, torch.bfloat16, torch.float16, torch.float64)
INTS = (torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64, torch.bool)


def _value_of(byte, dtype):
    """What `dtype` reads from memory filled with `byte`, from the byte pattern alone (struct, no torch)."""
    if dtype == torch.float64:
        return struct.unpack("<d", bytes([byte]) * 8)[0]
    if dtype == torch.float32:
        return struct.unpack("<f", bytes([byte]) * 4)[0]
    if dtype == torch.float16:
        return struct.unpack("<e", bytes([byte]) * 2)[0]
    return struct.unpack("<f", bytes([0, 0, byte, byte]))[0]          # bf16: the upper half of an fp32


def _allocators(dtype):
    like = torch.zeros(3, 5, dtype=dtype)
    return {"empty": lambda: torch.empty(3, 5, dtype=dtype), "empty_like": lambda: torch.empty_like(like),
            "new_empty": lambda: like.new_empty((7,)), "empty_strided_like": lambda: torch.empty_like(like.t()),
            "new_empty_dtype": lambda: torch.zeros(2, dtype=torch.int32).new_empty((4,), dtype=dtype)}


@pytest.mark.parametrize("dtype", FLOATS, ids=str)
def test_patterns(dtype):
    for name, alloc in _allocators(dtype).items():
        with P.poisoned(P.NAN_BYTE) as n:
            t = alloc()
        assert n[0] == 1 and t.dtype == dtype and bool(torch.isnan(t).all()), name
        with P.poisoned(P.HUGE_BYTE):
            t = alloc()
        want = _value_of(P.HUGE_BYTE, dtype)
        assert bool(torch.isfinite(t).all()) and bool((t.double() == want).all()), (name, want)
        assert abs(want / P.HUGE_VALUE[dtype] - 1) < 1e-6
    # the table of the module's docstring: NaN in all four / 1.3e36, 1.3e36, 61280, 6.5e286
    assert _value_of(P.NAN_BYTE, dtype) != _value_of(P.NAN_BYTE, dtype)
    lo, hi = {torch.float32: (1.3e36, 1.31e36), torch.bfloat16: (1.3e36, 1.31e36), torch.float16: (61280, 61280),
              torch.float64: (1e286, 1e287)}[dtype]
    assert lo <= _value_of(P.HUGE_BYTE, dtype) <= hi


@pytest.mark.parametrize("dtype", INTS, ids=str)
def test_integers_and_bools_are_untouched(dtype):
    """An index or a mask must never be poisoned.  What `torch.empty` holds is not defined, so the check is on the fill
    itself: storage pre-set to a known pattern stays as it was."""
    base = torch.full((16,), 1, dtype=dtype)
    before = base.clone()
    for byte in P.BYTES:
        assert P.fill_storage(base, byte) is base and torch.equal(base, before)
        with P.poisoned(byte):
            for alloc in _allocators(dtype).values():
                t = alloc()
                assert t.dtype == dtype
                if dtype == torch.bool:       # (a bool tensor read back from 0xFF / 0x7B bytes would not be 0 / 1)
                    continue
            i = torch.empty(0, dtype=dtype)       # empty storage: nothing to fill, nothing raised
            assert i.numel() == 0
    # a float tensor of no elements is fine too
    with P.poisoned(P.NAN_BYTE):
        assert torch.empty(0).numel() == 0 and torch.empty(0, 4).new_empty((0,)).numel() == 0


def test_fill_covers_the_whole_storage_and_needs_no_grad_mode():
    with P.poisoned(P.NAN_BYTE):
        t = torch.empty(4, 6).t()[1:3]                   # a view made afterwards still sees only poison
        assert bool(torch.isnan(t).all())
        g = torch.empty(5, requires_grad=True)           # a leaf that requires grad is filled without an autograd error
        assert g.requires_grad and g.grad_fn is None and bool(torch.isnan(g).all())
        buf = torch.zeros(8)
        torch.empty(8, out=buf)                          # out=: the caller's tensor, not a fresh workspace
        assert bool((buf == 0).all())


def test_restoration_also_after_an_exception():
    orig = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    with P.poisoned(P.NAN_BYTE):
        assert torch.empty is not orig[0] and torch.empty_like is not orig[1] and torch.Tensor.new_empty is not orig[2]
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == orig
    with pytest.raises(RuntimeError, match="boom"):
        with P.poisoned(P.HUGE_BYTE):
            raise RuntimeError("boom")
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == orig
    with P.plain() as n:
        torch.empty(3)
    assert n[0] == 0 and (torch.empty, torch.empty_like, torch.Tensor.new_empty) == orig


def test_nesting():
    orig = torch.empty
    with P.poisoned(P.NAN_BYTE):
        outer = torch.empty
        with P.poisoned(P.HUGE_BYTE):
            t = torch.empty(4)
            assert bool((t.double() == _value_of(P.HUGE_BYTE, torch.float32)).all())      # the inner fill stays
        assert torch.empty is outer
        assert bool(torch.isnan(torch.empty(4)).all())
    assert torch.empty is orig
    assert [label for label, _ in P.runs()] == ["plain", "0xFF", "0x7B"]


def test_the_package_allocates_through_the_patched_names():
    """One CPU-side helper of the package per name: `functional._dihedral_torch` (torch.empty_like), `_msrb_workspace`
    (Tensor.new_empty) and `ddp.GradSink.dest` (torch.empty)."""
    x = torch.arange(2 * 3 * 4 * 4, dtype=torch.float32).view(2, 3, 4, 4)
    for byte in P.BYTES:
        want = _value_of(byte, torch.float32)
        seen = lambda t: bool(torch.isnan(t).all()) if want != want else bool((t.double() == want).all())
        with P.poisoned(byte) as n:
            # (every element of this helper's allocation is overwritten: the manager's count shows the route)
            F._dihedral_torch(x, None, None, None, 1.0, False, None, 3)
            k = n[0]
            ws = TM._msrb_workspace(True, torch.zeros(1), 5)
            sink = ddp.GradSink(types.SimpleNamespace(arena=None, grad_sync=None), {}, torch.device("cpu"))
            g = sink.dest("w", (3, 2))
        assert k == 1, "functional._dihedral_torch does not reach torch.empty_like through the patched attribute"
        assert n[0] == 4
        assert ws[0].numel() == 128 * 5 and ws[1].numel() == 64 * 5 and seen(ws[0]) and seen(ws[1])
        assert g.shape == (3, 2) and seen(g)
    # and the filled helper still computes what it computed: every element of its result is written
    ref = F._dihedral_torch(x, None, None, None, 1.0, False, None, 5)
    with P.poisoned(P.NAN_BYTE):
        got = F._dihedral_torch(x, None, None, None, 1.0, False, None, 5)
    assert torch.equal(got, ref)
