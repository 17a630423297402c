"""The z-x slice adjoint's entries of the C-ABI (thz_asm_slice_adjoint_workspace_size,
thz_asm_slice_adjoint; library 0.6.0, ABI still 9) without a GPU: the symbols are exported and bound,
every validation path returns its code and leaves its word in thz_last_error() before any device
call, the workspace holds one plane's gradient spectrum and the rows' spectra only, and
propagate_zx refuses an unknown ``grad`` before anything touches a device.
"""
import ctypes

import pytest

LAM, DX = 2.998e8 / 300e9, 0.25e-3


def _zs(Z):
    return [0.02 + 0.1 * k / max(Z - 1, 1) for k in range(Z)]


def _desc(H=512, W=512, pad=256, unpad=True, Z=3, adjoint=True, **kw):
    from quantizationawarethzdoe_amd import _lib, propagation as P
    d = P._asm_desc(1, 1, H, W, pad, pad, unpad, 1, [LAM], [DX, DX], _zs(Z), adjoint)
    for k, v in kw.items():
        setattr(d, k, v)
    return _lib, d


def _adjoint(d, row, gout=8, gin=8, ws=8, ws_bytes=1 << 40):
    from quantizationawarethzdoe_amd import _lib
    code = _lib.lib().thz_asm_slice_adjoint(ctypes.byref(d), row, ctypes.c_void_p(gout), ctypes.c_void_p(gin),
                                            ctypes.c_void_p(ws), ctypes.c_size_t(ws_bytes), None)
    return code, _lib.lib().thz_last_error().decode()


def _size(d):
    from quantizationawarethzdoe_amd import _lib
    n = ctypes.c_size_t(0)
    code = _lib.lib().thz_asm_slice_adjoint_workspace_size(ctypes.byref(d), ctypes.byref(n))
    return code, n.value, _lib.lib().thz_last_error().decode()


def test_symbols_exported_bound_and_abi_still_9():
    from quantizationawarethzdoe_amd import _lib
    import quantizationawarethzdoe_amd as pkg
    h = _lib.lib()
    names = {"thz_asm_slice_adjoint_workspace_size", "thz_asm_slice_adjoint"}
    assert all(hasattr(h, n) for n in names) and names <= set(_lib.EXPORTED)
    assert h.thz_asm_slice_adjoint.argtypes is not None and len(h.thz_asm_slice_adjoint.argtypes) == 7
    assert h.thz_abi_version() == 9 == _lib.THZ_ABI_VERSION
    assert "0.6.0" in _lib.version() and pkg.__version__ == "0.6.0"


@pytest.mark.parametrize("Z", [3, 64, 256])
def test_workspace_is_one_plane_spectrum_and_the_rows_spectra(Z):
    """512^2 -> P = 1024: under T + Z (ncols rounded up to 16) 8 + 1 KiB, and under the full path's."""
    from quantizationawarethzdoe_amd import propagation as P
    _lib, d = _desc(Z=Z)
    code, n, _ = _size(d)
    assert code == _lib.THZ_OK
    ncols = P.asm_band_columns(1, 1, 512, 512, 256, 256, True, 1, [LAM], [DX, DX], _zs(Z))
    nc16 = (ncols + 15) // 16 * 16
    t = nc16 * 512 * 8
    assert Z * nc16 * 8 < n <= t + Z * nc16 * 8 + 1024, (Z, n, t, ncols)
    full = ctypes.c_size_t(0)
    assert _lib.lib().thz_asm_workspace_size(ctypes.byref(d), ctypes.byref(full)) == _lib.THZ_OK
    assert n < full.value, (Z, n, full.value)


@pytest.mark.parametrize("adjoint", [0, 2])
def test_descriptor_must_be_the_adjoint(adjoint):
    _lib, d = _desc(adjoint=adjoint)
    code, msg = _adjoint(d, 0)
    assert code == _lib.THZ_E_ARG and "adjoint" in msg
    code, _, msg = _size(d)
    assert code == _lib.THZ_E_ARG and "adjoint" in msg


@pytest.mark.parametrize("field, value, word", [("z_dev", 8, "z_dev"), ("window_mask", 8, "window mask")])
def test_unsupported_descriptor_fields(field, value, word):
    _lib, d = _desc(**{field: value})
    code, msg = _adjoint(d, 0)
    assert code == _lib.THZ_E_UNSUPPORTED and word in msg
    code, _, msg = _size(d)
    assert code == _lib.THZ_E_UNSUPPORTED and word in msg


@pytest.mark.parametrize("H, pad", [(100, 200), (100, 100), (500, 250), (512, 0)])
def test_padded_height_not_served(H, pad):
    _lib, d = _desc(H=H, W=H, pad=pad)
    code, msg = _adjoint(d, 0)
    assert code == _lib.THZ_E_UNSUPPORTED and "padded height" in msg and str(H + 2 * pad) in msg
    assert _size(d)[0] == _lib.THZ_E_UNSUPPORTED


@pytest.mark.parametrize("row", [-1, 512, 1 << 20])
def test_bad_row(row):
    _lib, d = _desc()
    code, msg = _adjoint(d, row)
    assert code == _lib.THZ_E_ARG and "row" in msg and "[0, 512)" in msg


def test_row_range_is_the_padded_plane_without_unpad():
    _lib, d = _desc(unpad=False)
    code, msg = _adjoint(d, 1024)
    assert code == _lib.THZ_E_ARG and "[0, 1024)" in msg
    assert _adjoint(d, 1023, ws_bytes=16)[0] == _lib.THZ_E_WORKSPACE  # the row is valid: the next check fails


@pytest.mark.parametrize("null", ["gout", "gin"])
def test_null_data_pointers(null):
    _lib, d = _desc()
    code, msg = _adjoint(d, 0, **{null: 0})
    assert code == _lib.THZ_E_ARG and "null" in msg


def test_null_descriptor_and_bytes():
    from quantizationawarethzdoe_amd import _lib
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    assert L.thz_asm_slice_adjoint_workspace_size(None, ctypes.byref(n)) == _lib.THZ_E_ARG
    assert b"null" in L.thz_last_error()
    _, d = _desc()
    assert L.thz_asm_slice_adjoint_workspace_size(ctypes.byref(d), None) == _lib.THZ_E_ARG
    assert b"null" in L.thz_last_error()
    assert L.thz_asm_slice_adjoint(None, 0, ctypes.c_void_p(8), ctypes.c_void_p(8), ctypes.c_void_p(8),
                                   ctypes.c_size_t(1 << 40), None) == _lib.THZ_E_ARG


def test_short_or_null_workspace():
    _lib, d = _desc()
    _, need, _ = _size(d)
    code, msg = _adjoint(d, 5, ws_bytes=need - 1)
    assert code == _lib.THZ_E_WORKSPACE and "workspace" in msg and str(need) in msg
    assert _adjoint(d, 5, ws=0)[0] == _lib.THZ_E_WORKSPACE


def test_slice_forward_still_refuses_the_adjoint_descriptor():
    _lib, d = _desc()
    code = _lib.lib().thz_asm_slice_forward(ctypes.byref(d), 0, ctypes.c_void_p(8), ctypes.c_void_p(8),
                                            ctypes.c_void_p(8), ctypes.c_size_t(1 << 40), None)
    assert code == _lib.THZ_E_UNSUPPORTED and b"adjoint" in _lib.lib().thz_last_error()


def test_propagate_zx_unknown_grad_is_a_value_error_without_gpu():
    import torch
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    from quantizationawarethzdoe_amd.Props.ASM_Prop import ASM_prop
    field = ElectricField(torch.ones(1, 1, 16, 12, dtype=torch.complex64), wavelengths=1e-3, spacing=[1e-3, 1e-3],
                          device="cpu")
    prop = ASM_prop(z_distance=0.1, device="cpu")
    with pytest.raises(ValueError, match="'planes' or 'slice'"):
        prop.propagate_zx(field, [0.1, 0.2], grad="both")
