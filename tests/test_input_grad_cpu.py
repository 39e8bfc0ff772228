"""CPU-side checks of the taxel gradient of the train step: the two stem data-gradient entry points are declared, bound
with the expected argument types and exported at an unchanged ABI, and they refuse bad arguments before any launch.
No compute calls."""
import ctypes
import os

from tactilesr_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tsr_stem_dgrad", "tsr_stem_dgrad_b16")
_P, _I = _lib._P, _lib._I


def test_header_declares_the_stem_dgrad_entry_points():
    with open(os.path.join(REPO, "include", "tactilesr_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert f"\nint {name}(" in header, name
    assert "model/tactileSR_model.py:35-37,60-61" in header


def test_library_binds_and_exports_the_stem_dgrad_entry_points_at_abi_24():
    lib = _lib.load()
    expect = [_P, _P, _I, _I, _I, _I, _I, _P, _I, _I, _I, _I, _P]
    for name in NAMES:
        assert _lib.SIGNATURES[name] == expect, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == expect, name
    assert _lib.ABI_VERSION == 24 and lib.tsr_abi_version() == 24


def test_stem_dgrad_rejects_bad_arguments():
    """Every call below fails its host-side argument check (the fake pointers are never dereferenced)."""
    lib = _lib.load()
    fake, null = ctypes.c_void_p(16), ctypes.c_void_p(0)
    for name in NAMES:
        fn = getattr(lib, name)
        ok = dict(w=fake, dz=fake, dz_ctot=64, dz_coff=0, hin=4, win=4, sf=10, dx=fake, dx_ctot=3, dx_coff=0, acc=0, B=1)

        def call(**kw):
            a = dict(ok, **kw)
            return fn(a["w"], a["dz"], a["dz_ctot"], a["dz_coff"], a["hin"], a["win"], a["sf"], a["dx"], a["dx_ctot"],
                      a["dx_coff"], a["acc"], a["B"], null)
        assert call(w=null) != 0
        assert call(dz=null) != 0
        assert call(dx=null) != 0
        assert call(B=0) != 0
        assert call(dz_ctot=72) != 0            # CB16: channel totals and offsets are multiples of 16
        assert call(dz_coff=8, dz_ctot=128) != 0
        assert call(dz_coff=16) != 0            # 64 channels past the end of the tensor
        assert call(dx_coff=1) != 0             # 3 channels past the end of dx
        assert call(dx_coff=-3) != 0
        assert call(hin=5) != 0 and call(win=0) != 0 and call(sf=0) != 0
        assert call(acc=2) != 0
        assert call(sf=2000) != 0               # tap tables beyond the LDS bound


def test_stem_wgrad_and_head_bwd_refuse_oversize_shapes_before_any_launch():
    """Shapes beyond the LDS bounds fail the host-side check (the fake pointers are never dereferenced): tsr_head_bwd at
    128 x 128 (scale_factor 32 on 4 x 4 taxels; at most 126 x 126), tsr_stem_wgrad with a row too wide for 160 KB."""
    lib = _lib.load()
    fake, null = ctypes.c_void_p(16), ctypes.c_void_p(0)
    amax = fake
    for H in (128, 160):
        assert lib.tsr_head_bwd(fake, fake, fake, 128, 128, fake, fake, 128, fake, 1, 1, H, H, amax, null) == 1
        assert lib.tsr_head_bwd_b16(fake, fake, fake, 128, 128, fake, fake, 128, fake, 1, 1, H, H, null) == 1
    for name in ("tsr_stem_wgrad", "tsr_stem_wgrad_b16"):
        fn = getattr(lib, name)
        assert fn(fake, 3, 0, 1, 4400, 1, fake, 64, 0, fake, 1, 1, null) == 1
        assert fn(fake, 3, 0, 4, 4, 0, fake, 64, 0, fake, 1, 1, null) == 1          # sf 0
        assert fn(fake, 3, 0, 4, 4, 10, fake, 64, 0, fake, 0, 1, null) == 1         # nsplit 0
