"""The thick-element DOE model without a GPU: the CPU restatement tests/thick_ref.py (slab thicknesses,
the thin limit against the oracle, passivity) and the C-ABI entries thz_thick_workspace_size /
thz_thick_forward (ABI 9, additive): the symbols are exported and every validation path returns its
code and leaves a message in thz_last_error() before any device call.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import thz_oracle as orc
from tests import table_ref as tr
from tests import thick_ref as th

C0 = 2.998e8
EPS, TAND = 2.66, 0.03


# ---------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 3, 4, 5, 16])
def test_slab_thicknesses_sum_to_the_clipped_height(S):
    T = 4e-3
    h = th.boundary_heights(8, 8, T, S, seed=S)
    dz = th.step_size(T, S)
    flat = h.reshape(-1)
    # the boundary values are in the map: 0, below 0, T, above T, and every z_s
    assert flat[0] == 0 and flat[1] < 0 and flat[2] == np.float32(T) and flat[3] > T
    for s in range(S):
        assert flat[4 + s] == np.float32(s * dz)
    d = th.slab_thicknesses(h, T, S)
    assert d.shape == (S, 8, 8) and float(d.min()) >= 0.0 and float(d.max()) <= dz
    want = h.double().clamp(0.0, float(np.float32(T)))
    assert float((d.sum(0) - want).abs().max()) <= 1e-17
    # with the base plate on the first slab: clamp(h, 0, T) + b
    b = th.BASE32
    total = (d[0] + b) + d[1:].sum(0)
    assert float((total - (want + b)).abs().max()) <= 1e-17
    # a slab is full below the relief, empty above it
    for s in range(S):
        assert torch.all(d[s][h.double() >= (s + 1) * dz] == dz) and torch.all(d[s][h.double() <= s * dz] == 0)
    # the fp32 slabs (z_s and dz rounded) agree to fp32 rounding of lengths of a few mm
    d32 = th.slab_thicknesses(h, T, S, torch.float32)
    assert d32.dtype == torch.float32 and float((d32.double() - d).abs().max()) <= 2.0 ** -24 * 2 * T


@pytest.mark.parametrize("case", [(1, 1, 32, 32, (32, 32), 1, (0.5e-3, 0.5e-3), "exact"),
                                  (2, 2, 24, 40, (6, 8), 1.5, (0.5e-3, 0.4e-3), "approx"),
                                  (1, 1, 21, 30, (21, 30), 1, (0.5e-3, 0.5e-3), None)],
                         ids=["32", "24x40_up", "21x30_nobl"])
def test_one_slice_reference_sign_is_modulate_then_asm(case):
    B, C, H, W, hw, s, sp, blt = case
    T = 3e-3
    lam = torch.tensor([np.float32(C0 / 280e9), np.float32(C0 / 320e9)][:C], dtype=torch.float64)
    ph, pw, Ph, Pw = orc.asm_padding(H, W, s, True)
    z = th.step_size(T, 1)
    Hc = orc.asm_transfer_function(Ph, Pw, lam, sp[0], sp[1], z, blt is not None, blt or "exact", rdt=torch.float64)
    x = torch.randn(B, C, H, W, dtype=torch.complex128, generator=torch.Generator().manual_seed(3))
    h = th.boundary_heights(hw[0], hw[1], T, 1, seed=5)
    got = th.thick_from_table(x, h, Hc, lam.tolist(), EPS, TAND, T, 1, ph, pw, sign=-1.0, base=orc.BASE_PLANE_THICKNESS)
    hc = h.double().clamp(0.0, float(np.float32(T)))
    eps64, tand64 = float(np.float32(EPS)), float(np.float32(TAND))
    mod = orc.doe_modulate(x, hc, lam, torch.tensor(eps64, dtype=torch.float64), torch.tensor(tand64, dtype=torch.float64))
    want = orc.asm_forward(mod, lam, sp, z, s, True, True, blt is not None, blt or "exact")
    assert got.shape == want.shape and got.dtype == torch.complex128
    assert float((got - want).norm() / want.norm()) <= 1e-12


def test_the_two_conventions_are_conjugate_screens():
    d = torch.rand(8, 8, dtype=torch.float64) * 1e-3
    lam = [1e-3, 1.1e-3]
    a = th.screen(d, lam, EPS, TAND, -1.0, True)
    b = th.screen(d, lam, EPS, TAND, 1.0, True)
    assert torch.equal(a.conj(), b) and a.shape == (2, 8, 8)
    lo = th.screen(d.float(), lam, EPS, TAND, 1.0, False, torch.complex64)
    assert lo.dtype == torch.complex64 and float((lo.to(tr.C128) - th.screen(d, lam, EPS, TAND, 1.0, False)).abs().max()) < 5e-6


@pytest.mark.parametrize("tand", [0.0, 0.03])
@pytest.mark.parametrize("sign", [-1.0, 1.0])
def test_output_energy_does_not_exceed_input_energy(tand, sign):
    H = W = 32
    T, S = 4e-3, 4
    lam = [float(np.float32(1e-3))]
    ph, pw, Ph, Pw = orc.asm_padding(H, W, 1, True)
    Hc = orc.asm_transfer_function(Ph, Pw, torch.tensor(lam, dtype=torch.float64), 1e-3, 1e-3, th.step_size(T, S), True,
                                   "exact", rdt=torch.float64)
    assert float(Hc.abs().max()) <= 1.0 + 1e-12
    x = torch.randn(1, 1, H, W, dtype=torch.complex128, generator=torch.Generator().manual_seed(1))
    h = th.boundary_heights(H, W, T, S, seed=2)
    out = th.thick_from_table(x, h, Hc, lam, EPS, tand, T, S, ph, pw, sign=sign)
    assert float(out.abs().pow(2).sum()) <= float(x.abs().pow(2).sum()) * (1 + 1e-12)


def test_restatement_is_differentiable_in_the_map():
    H = W = 16
    T, S = 3e-3, 3
    lam = [1e-3]
    ph, pw, Ph, Pw = orc.asm_padding(H, W, 1, True)
    Hc = orc.asm_transfer_function(Ph, Pw, torch.tensor(lam, dtype=torch.float64), 1e-3, 1e-3, th.step_size(T, S), True,
                                   "exact", rdt=torch.float64)
    x = torch.randn(1, 1, H, W, dtype=torch.complex128, generator=torch.Generator().manual_seed(1))
    h = (torch.rand(8, 8, generator=torch.Generator().manual_seed(2)) * T).requires_grad_(True)
    th.thick_from_table(x, h, Hc, lam, EPS, TAND, T, S, ph, pw).abs().pow(2).sum().backward()
    assert h.grad is not None and h.grad.shape == (8, 8) and float(h.grad.abs().max()) > 0


# ---------------------------------------------------------------------------------------------
# the C-ABI: descriptor and error codes (the built library, no device)
# ---------------------------------------------------------------------------------------------
def _desc(C=1, **kw):
    from quantizationawarethzdoe_amd import _lib
    wl = _lib.float_array([1e-3 * (1 + 0.1 * c) for c in range(C)])
    d = _lib.ThickDesc(B=1, C=C, H=512, W=512, pad_h=256, pad_w=256, bandlimit=1, hs=512, ws=512, slices=4,
                       thickness=4e-3, dx=1e-3, dy=1e-3, epsilon=2.66, tand=0.03, phase_sign=-1.0,
                       wavelengths=ctypes.cast(wl, ctypes.POINTER(ctypes.c_float)))
    d._keep = wl
    for k, v in kw.items():
        setattr(d, k, v)
    return _lib, d


def _forward(d, field=8, height=8, out=8, ws=8, ws_bytes=1 << 40):
    """The data pointers are never dereferenced: every call here fails its validation first."""
    from quantizationawarethzdoe_amd import _lib
    code = _lib.lib().thz_thick_forward(ctypes.byref(d), ctypes.c_void_p(field), ctypes.c_void_p(height),
                                        ctypes.c_void_p(out), ctypes.c_void_p(ws), ctypes.c_size_t(ws_bytes), None)
    return code, _lib.lib().thz_last_error().decode()


def _size(d):
    from quantizationawarethzdoe_amd import _lib
    n = ctypes.c_size_t(0)
    code = _lib.lib().thz_thick_workspace_size(ctypes.byref(d), ctypes.byref(n))
    return code, n.value, _lib.lib().thz_last_error().decode()


def test_symbols_exported_and_abi_9():
    from quantizationawarethzdoe_amd import _lib
    h = _lib.lib()
    assert hasattr(h, "thz_thick_workspace_size") and hasattr(h, "thz_thick_forward")
    assert {"thz_thick_workspace_size", "thz_thick_forward"} <= set(_lib.EXPORTED)
    assert h.thz_abi_version() == 9 == _lib.THZ_ABI_VERSION
    # thz_thick_desc: ten ints, six floats, one pointer
    assert ctypes.sizeof(_lib.ThickDesc) == 10 * 4 + 6 * 4 + ctypes.sizeof(ctypes.c_void_p)


@pytest.mark.parametrize("kw", [dict(B=0), dict(C=0), dict(H=0), dict(W=-1), dict(hs=0), dict(ws=0), dict(pad_h=-1),
                                dict(slices=0), dict(slices=-3), dict(thickness=0.0), dict(thickness=-1e-3),
                                dict(thickness=float("nan")), dict(phase_sign=0.0), dict(phase_sign=0.5),
                                dict(phase_sign=2.0), dict(phase_sign=float("nan")), dict(bandlimit=3), dict(dx=0.0),
                                dict(epsilon=0.0)],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_argument_errors(kw):
    _lib, d = _desc(**kw)
    for code, msg in (_forward(d), _size(d)[::2]):
        assert code == _lib.THZ_E_ARG and msg, (kw, code, msg)


def test_null_descriptor_bytes_and_pointers():
    from quantizationawarethzdoe_amd import _lib
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    assert L.thz_thick_workspace_size(None, ctypes.byref(n)) == _lib.THZ_E_ARG and b"null" in L.thz_last_error()
    _, d = _desc()
    assert L.thz_thick_workspace_size(ctypes.byref(d), None) == _lib.THZ_E_ARG and b"null" in L.thz_last_error()
    assert L.thz_thick_forward(None, ctypes.c_void_p(8), ctypes.c_void_p(8), ctypes.c_void_p(8), ctypes.c_void_p(8),
                               ctypes.c_size_t(1 << 40), None) == _lib.THZ_E_ARG
    for null in ("field", "height", "out"):
        code, msg = _forward(d, **{null: 0})
        assert code == _lib.THZ_E_ARG and "null" in msg
    _, d = _desc()
    d.wavelengths = ctypes.POINTER(ctypes.c_float)()
    for code, msg in (_forward(d), _size(d)[::2]):
        assert code == _lib.THZ_E_ARG and "null" in msg
    _, d = _desc()
    d._keep[0] = 0.0
    assert _size(d)[0] == _lib.THZ_E_ARG


@pytest.mark.parametrize("kw", [dict(H=100, W=100, pad_h=100, pad_w=100),      # the 300-point notebook geometry
                                dict(H=16, W=16, pad_h=8, pad_w=8),            # 32 < 64
                                dict(H=8192, W=8192, pad_h=4096, pad_w=4096),  # 16384 > 8192
                                dict(H=512, pad_h=256, W=500, pad_w=250),      # one side no power of two
                                dict(W=512, pad_w=256, H=96, pad_h=48),
                                dict(slices=257), dict(C=65)],
                         ids=["300", "32", "16384", "1000w", "192h", "slices257", "C65"])
def test_unsupported_geometries(kw):
    _lib, d = _desc(**kw)
    for code, msg in (_forward(d), _size(d)[::2]):
        assert code == _lib.THZ_E_UNSUPPORTED and msg, (kw, code, msg)


def test_argument_errors_come_before_unsupported_and_workspace():
    _lib, d = _desc(H=100, W=100, pad_h=100, pad_w=100, slices=0)
    assert _forward(d, ws=0)[0] == _lib.THZ_E_ARG
    _lib, d = _desc(H=100, W=100, pad_h=100, pad_w=100)
    assert _forward(d, ws=0)[0] == _lib.THZ_E_UNSUPPORTED


@pytest.mark.parametrize("shape", [(1, 1, 512, 512, 256, 256), (2, 3, 64, 32, 32, 16), (1, 1, 32, 32, 16, 16),
                                   (1, 2, 2048, 4096, 1024, 2048), (1, 1, 50, 8, 7, 28)])
def test_workspace_is_the_window_rows_spectra_and_one_table(shape):
    B, C, H, W, ph, pw = shape
    _lib, d = _desc(C=C, B=B, H=H, W=W, pad_h=ph, pad_w=pw, hs=H, ws=W)
    code, n, msg = _size(d)
    assert code == _lib.THZ_OK, msg
    Ph, Pw = H + 2 * ph, W + 2 * pw
    rows = H + (1 if (H * 128) % 4096 == 0 else 0)   # a block of H rows off a multiple of 4096 B
    r256 = lambda v: (v + 255) // 256 * 256
    assert n == r256(8 * B * C * Pw * rows) + r256(8 * C * Ph * Pw), (shape, n)
    # no growth with the slice count: one table serves every slab
    d.slices = 256
    assert _size(d)[1] == n
    code, msg = _forward(d, ws_bytes=n - 1)
    assert code == _lib.THZ_E_WORKSPACE and str(n) in msg
    code, msg = _forward(d, ws=0)
    assert code == _lib.THZ_E_WORKSPACE and str(n) in msg


def test_python_argument_errors_without_gpu():
    from quantizationawarethzdoe_amd import optics
    from quantizationawarethzdoe_amd.Components.ThickDOE import ThickDOEElement
    x = torch.ones(1, 1, 32, 32, dtype=torch.complex64)
    h = torch.zeros(32, 32)
    with pytest.raises(RuntimeError, match="no CPU compute path"):
        optics.thick_doe(x, h, [1e-3], 1e-3, EPS, TAND, 4e-3, 4)
    assert optics.thick_doe_native(32, 32, 16, 16, 4) and optics.thick_doe_native(64, 32, 32, 16, 256)
    assert not optics.thick_doe_native(100, 100, 100, 100, 4) and not optics.thick_doe_native(32, 32, 16, 16, 257)
    assert not optics.thick_doe_native(8192, 8192, 4096, 4096, 1) and not optics.thick_doe_native(16, 16, 8, 8, 1)
    with pytest.raises(ValueError, match="convention"):
        ThickDOEElement(h, 4e-3, 4, [EPS, TAND], convention="other", device="cpu")
    with pytest.raises(ValueError, match="slices"):
        ThickDOEElement(h, 4e-3, 0, [EPS, TAND], device="cpu")
    el = ThickDOEElement(h, 4e-3, 4, [EPS, TAND], device="cpu")
    assert el.height_map.shape == (32, 32) and not el.height_map.requires_grad and el.method == "auto"
    import quantizationawarethzdoe_amd as pkg
    pkg.install_reference_aliases()
    from Components.ThickDOE import ThickDOEElement as aliased
    assert aliased is ThickDOEElement
