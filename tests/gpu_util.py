"""What the GPU tests share besides the parity rule (tests/parity.py): the device, seeded inputs, placement at a chosen
alignment, bit comparison, launch counts and the workspace-size ABI call.

Plain helper module: no test, no fixture.
"""
import ctypes

import pytest
import torch

C0 = 2.998e8   # the suite's speed of light: wavelengths are C0 / f rounded to float32
C64 = torch.complex64


def dev():
    """cuda:0; skips the calling test without a GPU (in a module marked ``gpu`` the collection hook already has)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    return torch.device("cuda:0")


def f32(v):
    """v rounded to float32, as a Python float"""
    return float(torch.tensor(v, dtype=torch.float32))


def lam_ghz(ghz):
    """the float32 wavelength of a frequency in GHz"""
    return f32(C0 / (ghz * 1e9))


def white_cpu(shape, seed):
    """Seeded complex white noise from the CPU generator: drawn in complex128, rounded to complex64."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, dtype=torch.complex128, generator=g).to(C64)


def white_gpu(shape, seed, dtype=C64):
    """Seeded complex white noise drawn on cuda:0 by the device generator."""
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    return torch.randn(*shape, dtype=dtype, device="cuda:0", generator=g)


def launches(fn, names):
    """(result of fn(), launches of each timed kernel family of ``names``)"""
    from quantizationawarethzdoe_amd import _lib
    _lib.timing_enable(True)
    try:
        _lib.timing_reset()
        out = fn()
        return out, tuple(_lib.timing_read(n)[1] for n in names)
    finally:
        _lib.timing_enable(False)
        _lib.timing_reset()


def place(t, offset=0):
    """A contiguous device copy of ``t`` whose pointer is 16-byte aligned (offset 0) or ``offset`` elements past such an
    address (16-byte elements stay aligned)."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=dev())
    assert buf.data_ptr() % 16 == 0
    v = buf[offset:offset + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and (v.data_ptr() % 16 == 0) == (offset == 0 or t.element_size() == 16)
    return v.detach()


def bits(a, b):
    """Same dtype, shape and bit pattern (+0.0 is not -0.0; equal NaN payloads are equal)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.is_complex():
        a, b = torch.view_as_real(a), torch.view_as_real(b)
    wide = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return bool((a.view(wide) == b.view(wide)).all())


def workspace_size(symbol, desc):
    """(code, bytes, last error) of the library's ``symbol``(&desc, &bytes)"""
    from quantizationawarethzdoe_amd import _lib
    n = ctypes.c_size_t(0)
    code = getattr(_lib.lib(), symbol)(ctypes.byref(desc), ctypes.byref(n))
    return code, n.value, _lib.lib().thz_last_error().decode()
