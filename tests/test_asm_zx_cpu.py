"""The z-x slice entries of the C-ABI (thz_asm_slice_workspace_size, thz_asm_slice_forward; ABI 9)
without a GPU: the symbols are exported, the ABI version matches the bindings, and every
validation path returns its code and leaves a message in thz_last_error() before any device call.
"""
import ctypes

import pytest


def _desc(H=512, W=512, pad=256, unpad=True, Z=3, **kw):
    from quantizationawarethzdoe_amd import _lib, propagation as P
    d = P._asm_desc(1, 1, H, W, pad, pad, unpad, 1, [2.998e8 / 300e9], [0.25e-3, 0.25e-3],
                    [0.02 + 0.01 * k for k in range(Z)], False)
    for k, v in kw.items():
        setattr(d, k, v)
    return _lib, d


def _forward(d, row, inp=8, out=8, ws=8, ws_bytes=1 << 40):
    from quantizationawarethzdoe_amd import _lib
    code = _lib.lib().thz_asm_slice_forward(ctypes.byref(d), row, ctypes.c_void_p(inp), ctypes.c_void_p(out),
                                            ctypes.c_void_p(ws), ctypes.c_size_t(ws_bytes), None)
    return code, _lib.lib().thz_last_error().decode()


def _size(d):
    from quantizationawarethzdoe_amd import _lib
    n = ctypes.c_size_t(0)
    code = _lib.lib().thz_asm_slice_workspace_size(ctypes.byref(d), ctypes.byref(n))
    return code, n.value, _lib.lib().thz_last_error().decode()


def test_symbols_exported_and_abi_9():
    from quantizationawarethzdoe_amd import _lib
    h = _lib.lib()
    assert hasattr(h, "thz_asm_slice_workspace_size") and hasattr(h, "thz_asm_slice_forward")
    assert {"thz_asm_slice_workspace_size", "thz_asm_slice_forward"} <= set(_lib.EXPORTED)
    assert h.thz_abi_version() == 9 == _lib.THZ_ABI_VERSION


def test_workspace_holds_T_and_V_only():
    """512^2 -> P = 1024: T [ncb 16][H] and V [min(Z, 64)][ncols], nothing of a plane's size per z."""
    from quantizationawarethzdoe_amd import propagation as P
    for Z in (3, 64, 200):
        _lib, d = _desc(Z=Z)
        code, n, _ = _size(d)
        assert code == _lib.THZ_OK
        ncols = P.asm_band_columns(1, 1, 512, 512, 256, 256, True, 1, [2.998e8 / 300e9], [0.25e-3, 0.25e-3],
                                   [0.02 + 0.01 * k for k in range(Z)])
        t = (ncols + 15) // 16 * 16 * 512 * 8
        v = min(Z, 64) * ncols * 8   # V does not grow past 64 planes
        assert t + v <= n <= t + v + 512, (Z, n, t, v)   # two 256-byte alignments
        full = ctypes.c_size_t(0)
        assert _lib.lib().thz_asm_workspace_size(ctypes.byref(d), ctypes.byref(full)) == _lib.THZ_OK
        assert n < full.value and n - t < 512 * 512 * 8   # less than one plane beside T


@pytest.mark.parametrize("row", [-1, 512, 1 << 20])
def test_bad_row_is_an_argument_error(row):
    _lib, d = _desc()
    code, msg = _forward(d, row)
    assert code == _lib.THZ_E_ARG and "row" in msg and "[0, 512)" in msg


def test_row_range_is_the_padded_plane_without_unpad():
    _lib, d = _desc(unpad=False)
    code, msg = _forward(d, 1024)
    assert code == _lib.THZ_E_ARG and "[0, 1024)" in msg
    # row 1023 is valid there: the next check (the workspace) is the one that fails
    code, msg = _forward(d, 1023, ws_bytes=16)
    assert code == _lib.THZ_E_WORKSPACE


@pytest.mark.parametrize("null", ["inp", "out"])
def test_null_data_pointers(null):
    _lib, d = _desc()
    code, msg = _forward(d, 0, **{null: 0})
    assert code == _lib.THZ_E_ARG and "null" in msg


def test_null_descriptor_and_bytes():
    from quantizationawarethzdoe_amd import _lib
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    assert L.thz_asm_slice_workspace_size(None, ctypes.byref(n)) == _lib.THZ_E_ARG
    assert b"null" in L.thz_last_error()
    _, d = _desc()
    assert L.thz_asm_slice_workspace_size(ctypes.byref(d), None) == _lib.THZ_E_ARG
    assert b"null" in L.thz_last_error()
    assert L.thz_asm_slice_forward(None, 0, ctypes.c_void_p(8), ctypes.c_void_p(8), ctypes.c_void_p(8),
                                   ctypes.c_size_t(1 << 40), None) == _lib.THZ_E_ARG


@pytest.mark.parametrize("field, value, word", [
    ("adjoint", 1, "adjoint"),
    ("z_dev", 8, "z_dev"),
    ("window_mask", 8, "window mask"),
])
def test_unsupported_descriptor_fields(field, value, word):
    _lib, d = _desc(**{field: value})
    code, msg = _forward(d, 0)
    assert code == _lib.THZ_E_UNSUPPORTED and word in msg
    code, _, msg = _size(d)
    assert code == _lib.THZ_E_UNSUPPORTED and word in msg


@pytest.mark.parametrize("H, pad", [(100, 200), (100, 100), (500, 250), (512, 0), (300, 106)])
def test_padded_height_not_served_natively(H, pad):
    """The notebook's own P = 500 (100-pixel field, padding scale 4), the 300-point layers, and
    powers of two below 1024: the caller slices thz_asm_forward's planes instead."""
    _lib, d = _desc(H=H, W=H, pad=pad)
    code, msg = _forward(d, 0)
    assert code == _lib.THZ_E_UNSUPPORTED and "padded height" in msg and str(H + 2 * pad) in msg
    assert _size(d)[0] == _lib.THZ_E_UNSUPPORTED


def test_short_or_null_workspace():
    _lib, d = _desc()
    _, need, _ = _size(d)
    code, msg = _forward(d, 5, ws_bytes=need - 1)
    assert code == _lib.THZ_E_WORKSPACE and str(need) in msg
    code, msg = _forward(d, 5, ws=0)
    assert code == _lib.THZ_E_WORKSPACE


def test_propagate_zx_argument_errors_without_gpu():
    """row and axis are checked before anything touches a device."""
    import torch
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    from quantizationawarethzdoe_amd.Props.ASM_Prop import ASM_prop
    field = ElectricField(torch.ones(1, 1, 16, 12, dtype=torch.complex64), wavelengths=1e-3, spacing=[1e-3, 1e-3],
                          device="cpu")
    prop = ASM_prop(z_distance=0.1, device="cpu")
    with pytest.raises(ValueError, match=r"\[0, 16\)"):
        prop.propagate_zx(field, [0.1, 0.2], row=16)
    with pytest.raises(ValueError, match=r"\[0, 12\)"):
        prop.propagate_zx(field, [0.1, 0.2], row=-1, axis="y")
    with pytest.raises(ValueError, match="'x' or 'y'"):
        prop.propagate_zx(field, [0.1, 0.2], axis="z")
