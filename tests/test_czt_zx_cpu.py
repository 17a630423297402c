"""The CZT z-x slice entries of the C-ABI (thz_czt_slice_workspace_size, thz_czt_slice_forward; ABI 9,
additive) without a GPU: the symbols are exported, every validation path returns its code and leaves
a message in thz_last_error() before any device call, the workspace holds a chunk's tables and
column sums only, and the decomposition the kernels implement equals the oracle's planes in fp64.
"""
import ctypes
import math

import pytest
import torch

# (H, W, out, C, B, (dx, dy), (odx, ody)): the geometries of tests/test_czt_zx_gpu.py
GEOMETRIES = [
    (72, 100, 40, 2, 2, (0.25e-3, 0.3e-3), (0.1e-3, 0.12e-3)),
    (48, 48, 64, 1, 1, (0.25e-3, 0.25e-3), (0.05e-3, 0.05e-3)),
    (130, 70, 33, 3, 1, (0.25e-3, 0.25e-3), (0.1e-3, 0.1e-3)),
    (20, 24, 20, 1, 2, (0.5e-3, 0.5e-3), (0.2e-3, 0.2e-3)),
]


def _desc(H=2048, W=2048, out=512, C=2, B=1, Z=3, row=5, **kw):
    from quantizationawarethzdoe_amd import _lib, propagation as P
    d = P._czt_slice_desc(B, C, H, W, out, out, (0.25e-3, 0.25e-3), 0.05e-3, 0.05e-3,
                          [1e-3 * (1 + 0.1 * c) for c in range(C)], [0.02 + 0.001 * k for k in range(Z)], row)
    for k, v in kw.items():
        setattr(d, k, v)
    return _lib, d


def _forward(d, inp=8, out=8, ws=8, ws_bytes=1 << 40):
    from quantizationawarethzdoe_amd import _lib
    code = _lib.lib().thz_czt_slice_forward(ctypes.byref(d), ctypes.c_void_p(inp), ctypes.c_void_p(out),
                                            ctypes.c_void_p(ws), ctypes.c_size_t(ws_bytes), None)
    return code, _lib.lib().thz_last_error().decode()


def _size(d):
    from quantizationawarethzdoe_amd import _lib
    n = ctypes.c_size_t(0)
    code = _lib.lib().thz_czt_slice_workspace_size(ctypes.byref(d), ctypes.byref(n))
    return code, n.value, _lib.lib().thz_last_error().decode()


def test_symbols_exported_and_abi_9():
    from quantizationawarethzdoe_amd import _lib
    h = _lib.lib()
    assert hasattr(h, "thz_czt_slice_workspace_size") and hasattr(h, "thz_czt_slice_forward")
    assert {"thz_czt_slice_workspace_size", "thz_czt_slice_forward"} <= set(_lib.EXPORTED)
    assert h.thz_abi_version() == 9 == _lib.THZ_ABI_VERSION


@pytest.mark.parametrize("row", [-1, 512, 1 << 20])
def test_bad_row_is_an_argument_error(row):
    _lib, d = _desc(row=row)
    for code, msg in (_forward(d), _size(d)[::2]):
        assert code == _lib.THZ_E_ARG and "row" in msg and "[0, 512)" in msg


@pytest.mark.parametrize("Z", [0, 257])
def test_plane_count_outside_1_to_max_z(Z):
    _lib, d = _desc()
    assert _lib.THZ_MAX_Z == 256
    d.Z = Z
    for code, msg in (_forward(d), _size(d)[::2]):
        assert code == _lib.THZ_E_ARG and "Z=" in msg and "256" in msg


def test_null_descriptor_bytes_and_data():
    from quantizationawarethzdoe_amd import _lib
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    assert L.thz_czt_slice_workspace_size(None, ctypes.byref(n)) == _lib.THZ_E_ARG
    assert b"null" in L.thz_last_error()
    _, d = _desc()
    assert L.thz_czt_slice_workspace_size(ctypes.byref(d), None) == _lib.THZ_E_ARG
    assert b"null" in L.thz_last_error()
    assert L.thz_czt_slice_forward(None, ctypes.c_void_p(8), ctypes.c_void_p(8), ctypes.c_void_p(8),
                                   ctypes.c_size_t(1 << 40), None) == _lib.THZ_E_ARG
    assert b"null" in L.thz_last_error()
    for null in ("inp", "out"):
        code, msg = _forward(d, **{null: 0})
        assert code == _lib.THZ_E_ARG and "null" in msg
    for field in ("z", "wavelengths"):
        _, d = _desc()
        setattr(d, field, ctypes.POINTER(ctypes.c_float)())
        code, msg = _forward(d)
        assert code == _lib.THZ_E_ARG and "null" in msg


def test_shape_rules_of_the_planes():
    """czt_validate's rules, unchanged: the slice accepts exactly the geometries the planes accept."""
    _lib, d = _desc()
    d.outW = 500
    code, msg = _forward(d)
    assert code == _lib.THZ_E_ARG and "square" in msg
    _lib, d = _desc(H=33, W=33, out=32, row=0)   # m + M - 1 = 64
    for code, msg in (_forward(d), _size(d)[::2]):
        assert code == _lib.THZ_E_ARG and "power of two" in msg and "64" in msg
    _lib, d = _desc(C=65)
    assert _forward(d)[0] == _lib.THZ_E_UNSUPPORTED
    _lib, d = _desc(H=16000, W=16000, out=512)   # np2 = 32768
    code, msg = _forward(d)
    assert code == _lib.THZ_E_UNSUPPORTED and "16384" in msg
    _lib, d = _desc(B=0)
    assert _forward(d)[0] == _lib.THZ_E_ARG


def test_short_or_null_workspace():
    _lib, d = _desc()
    _, need, _ = _size(d)
    code, msg = _forward(d, ws_bytes=need - 1)
    assert code == _lib.THZ_E_WORKSPACE and str(need) in msg
    code, msg = _forward(d, ws=0)
    assert code == _lib.THZ_E_WORKSPACE and str(need) in msg


def test_workspace_holds_a_chunk_of_tables_and_column_sums():
    """(2048, 2048) -> 512, C = 2, B = 1: below the planes' workspace, below one V intermediate, and
    no growth with Z past the library's z-chunk (16 planes)."""
    sizes = {}
    for Z in (1, 16, 64, 200):
        _lib, d = _desc(Z=Z)
        code, n, _ = _size(d)
        assert code == _lib.THZ_OK
        sizes[Z] = n
        plane = _lib.CztDesc(B=1, C=2, H=2048, W=2048, outH=512, outW=512, dx=d.dx, dy=d.dy, odx=d.odx, ody=d.ody,
                             z=0.02, wavelengths=d.wavelengths, adjoint=0)
        full = ctypes.c_size_t(0)
        assert _lib.lib().thz_czt_workspace_size(ctypes.byref(plane), ctypes.byref(full)) == _lib.THZ_OK
        assert n < full.value, (Z, n, full.value)
        assert n < 1 * 2 * 2048 * 512 * 8, (Z, n)   # one V intermediate, B C H outH complex64
        # the header's formula: tables per (plane, wavelength) + at most 8 partial sums of S
        zc = min(Z, 16)
        tables = 8 * zc * 2 * (2048 + 512 + 4096 + 2048 + 32)
        assert tables + 8 * zc * 2 * 2048 <= n <= tables + 8 * 8 * zc * 2 * 2048 + 512, (Z, n)
    assert sizes[1] < sizes[16] == sizes[64] == sizes[200]


def test_propagate_zx_argument_errors_without_gpu():
    """row and axis are checked before anything touches a device."""
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    from quantizationawarethzdoe_amd.Props.CZT_Prop import CZT_prop, VCZT_prop
    field = ElectricField(torch.ones(1, 1, 16, 12, dtype=torch.complex64), wavelengths=1e-3, spacing=[1e-3, 1e-3],
                          device="cpu")
    for cls in (CZT_prop, VCZT_prop):
        prop = cls(z_distance=0.1, device="cpu")
        with pytest.raises(ValueError, match=r"\[0, 20\)"):
            prop.propagate_zx(field, [0.1, 0.2], row=20, outputHeight=20, outputWidth=20)
        with pytest.raises(ValueError, match=r"\[0, 20\)"):
            prop.propagate_zx(field, [0.1, 0.2], row=-1, axis="y", outputHeight=20, outputWidth=20)
        with pytest.raises(ValueError, match=r"\[0, 12\)"):
            prop.propagate_zx(field, [0.1, 0.2], row=12)   # the default output grid is the input's: outW = W
        with pytest.raises(ValueError, match="'x' or 'y'"):
            prop.propagate_zx(field, [0.1, 0.2], axis="z")


# ---------------------------------------------------------------------------------------------
# The decomposition the kernels implement, restated in torch (fp64) and held against the oracle
# ---------------------------------------------------------------------------------------------
def slice_decomposition(data, lam, spacing, z, out, odx, ody, p):
    """Row p of czt_forward's [B, C, outW, outH] plane without pass B's transform:
    coef[h] = preB[h] gB[p + H - h] (gB = 0 from ntab on), S[w] = sum_h E F coef, then pass A
    (oracle _bluestein) on S and the factors cst F0(x_out[p], y_out[q]) postB[p]."""
    from oracle import thz_oracle as orc
    B, C, H, W = data.shape
    dx, dy = spacing
    M = out
    xi = torch.linspace(-H * dx / 2, H * dx / 2, H)
    yi = torch.linspace(-W * dy / 2, W * dy / 2, W)
    imx, imy = torch.meshgrid(xi, yi, indexing="ij")
    xo = torch.linspace(-out * odx / 2, out * odx / 2, out)
    yo = torch.linspace(-out * ody / 2, out * ody / 2, out)
    Dm = lam[None, :, None, None] * z / dx
    fx1, fx2 = xo[0] + Dm / 2, xo[-1] + Dm / 2
    fy1, fy2 = yo[0] + Dm / 2, yo[-1] + Dm / 2
    # pass B (H axis, fy, M = outW): the kernels' table formulas (czt_tables / czt_slice_tables)
    D1 = (fy1 + (M * Dm + fy2 - fy1) / (2 * M)).reshape(C, 1)
    D2 = (fy2 + (M * Dm + fy2 - fy1) / (2 * M)).reshape(C, 1)
    dm = Dm.reshape(C, 1)
    thA = 2 * math.pi * D1 / dm
    thW = -2 * math.pi * (D1 - D2) / (M * dm)
    h = torch.arange(H, dtype=torch.float64)[None, :]
    pre = torch.exp(1j * (-thA * h + thW * h * h / 2))
    t = p + H - h
    ntab = min(H + M, H + max(M - 1, H - 1))
    g = torch.where(t < ntab, torch.exp(-1j * thW * (t - H + 1) ** 2 / 2), torch.zeros((), dtype=torch.complex128))
    coef = pre * g                                                     # [C, H]
    ell = p / M * (D2 - D1) + D1
    postB = torch.exp(1j * (thW * p * p / 2 - 2 * math.pi * ell * (-H / 2 + 0.5) / dm))   # [C, 1], no 1/nrm
    F = orc._rs_kernel(z, imx, imy, lam)
    S = (data * F * coef[None, :, :, None]).sum(-2)                    # [B, C, W]
    U = orc._bluestein(S[..., None], fx1, fx2, Dm, out)                # pass A along W: [B, C, 1, outH]
    F0 = orc._rs_kernel(z, xo[p].expand(1, out), yo[None, :], lam)     # [1, C, 1, outH]
    res = F0 * U * postB[None, :, :, None] * z * odx * ody * lam[None, :, None, None]
    return res[:, :, 0, :], bool((t >= ntab).any())


@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: f"{g[0]}x{g[1]}to{g[2]}")
def test_decomposition_equals_the_oracle_planes_fp64(geo):
    from oracle import thz_oracle as orc
    H, W, out, C, B, spacing, (odx, ody) = geo
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        g = torch.Generator().manual_seed(H * 1000 + W)
        data = torch.randn(B, C, H, W, dtype=torch.complex128, generator=g)
        lam = torch.tensor([1e-3 * (1 + 0.1 * c) for c in range(C)])
        hit_ntab = False
        for z in (0.03, 0.07):
            ref = orc.czt_forward(data, lam, list(spacing), z, out, out, odx, ody)
            for p in (0, out // 2, out - 1):
                got, cut = slice_decomposition(data, lam, spacing, z, out, odx, ody, p)
                hit_ntab |= cut
                want = ref[:, :, p, :]
                rel = float((got - want).norm() / want.norm())
                assert rel <= 1e-12, (geo, z, p, rel)
        # out >= input: row out - 1 meets the term (l = M - 1, j = 0) that falls on t = ntab
        assert hit_ntab == (out >= H)
    finally:
        torch.set_default_dtype(old)
