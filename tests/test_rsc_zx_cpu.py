"""The RSC / VRS z-x slice entries of the C-ABI (thz_rsc_slice_workspace_size, thz_rsc_slice_forward;
ABI 9, additive) without a GPU: the symbols are exported, every validation path returns its code and
leaves a message in thz_last_error() before any device call, the workspace holds the input rows'
spectra and one chunk's partial sums only, and the identity the kernels implement -- a sum of H
one-dimensional convolutions for one output row -- equals the oracle's planes in fp64.
"""
import ctypes

import pytest
import torch

# (H, W, C, B, (dx, dy)): the scalar geometries of tests/test_rsc_zx_gpu.py and two tiny ones
GEOMETRIES = [
    (72, 100, 2, 1, (0.25e-3, 0.3e-3)),
    (33, 47, 1, 2, (0.25e-3, 0.25e-3)),
    (130, 70, 3, 1, (0.25e-3, 0.25e-3)),
    (20, 24, 1, 1, (0.5e-3, 0.5e-3)),
    (2, 3, 1, 1, (0.5e-3, 0.5e-3)),
]
ZS = (0.030, 0.0725)


def _desc(H=1024, W=1024, C=2, B=1, Z=3, row=5, vectorial=0, **kw):
    from quantizationawarethzdoe_amd import _lib
    wl = _lib.float_array([1e-3 * (1 + 0.1 * c) for c in range(C)])
    zv = _lib.float_array([0.02 + 0.001 * k for k in range(Z)])
    d = _lib.RscSliceDesc(B=B, C=C, H=H, W=W, vectorial=vectorial, dx=0.25e-3, dy=0.25e-3, Z=Z,
                          z=ctypes.cast(zv, ctypes.POINTER(ctypes.c_float)),
                          wavelengths=ctypes.cast(wl, ctypes.POINTER(ctypes.c_float)), row=row)
    d._keep = (wl, zv)
    for k, v in kw.items():
        setattr(d, k, v)
    return _lib, d


def _forward(d, inp=8, out=8, ws=8, ws_bytes=1 << 40):
    """The data pointers are never dereferenced: every call here fails its validation first."""
    from quantizationawarethzdoe_amd import _lib
    code = _lib.lib().thz_rsc_slice_forward(ctypes.byref(d), ctypes.c_void_p(inp), ctypes.c_void_p(out),
                                            ctypes.c_void_p(ws), ctypes.c_size_t(ws_bytes), None)
    return code, _lib.lib().thz_last_error().decode()


def _size(d):
    from quantizationawarethzdoe_amd import _lib
    n = ctypes.c_size_t(0)
    code = _lib.lib().thz_rsc_slice_workspace_size(ctypes.byref(d), ctypes.byref(n))
    return code, n.value, _lib.lib().thz_last_error().decode()


def test_symbols_exported_and_abi_9():
    from quantizationawarethzdoe_amd import _lib
    h = _lib.lib()
    assert hasattr(h, "thz_rsc_slice_workspace_size") and hasattr(h, "thz_rsc_slice_forward")
    assert {"thz_rsc_slice_workspace_size", "thz_rsc_slice_forward"} <= set(_lib.EXPORTED)
    assert h.thz_abi_version() == 9 == _lib.THZ_ABI_VERSION


@pytest.mark.parametrize("row", [-1, 1024, 1 << 20])
def test_bad_row_is_an_argument_error(row):
    _lib, d = _desc(row=row)
    for code, msg in (_forward(d), _size(d)[::2]):
        assert code == _lib.THZ_E_ARG and "row" in msg and "[0, 1024)" in msg


def test_odd_height_keeps_h_minus_one_rows():
    """Ph - H = 2 floor(H / 2): 32 rows for H = 33, none for H = 1."""
    _lib, d = _desc(H=33, W=47, row=32)
    code, msg = _forward(d)
    assert code == _lib.THZ_E_ARG and "[0, 32)" in msg
    _lib, d = _desc(H=33, W=47, row=31)
    assert _size(d)[0] == _lib.THZ_OK
    _lib, d = _desc(H=1, W=8, row=0)
    code, msg = _forward(d)
    assert code == _lib.THZ_E_ARG and "[0, 0)" in msg


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
    assert L.thz_rsc_slice_workspace_size(None, ctypes.byref(n)) == _lib.THZ_E_ARG
    assert b"null" in L.thz_last_error()
    _, d = _desc()
    assert L.thz_rsc_slice_workspace_size(ctypes.byref(d), None) == _lib.THZ_E_ARG
    assert b"null" in L.thz_last_error()
    assert L.thz_rsc_slice_forward(None, ctypes.c_void_p(8), ctypes.c_void_p(8), ctypes.c_void_p(8),
                                   ctypes.c_size_t(1 << 40), None) == _lib.THZ_E_ARG
    assert b"null" in L.thz_last_error()
    for null in ("inp", "out"):
        code, msg = _forward(d, **{null: 0})
        assert code == _lib.THZ_E_ARG and "null" in msg
    for field in ("z", "wavelengths"):
        _, d = _desc()
        setattr(d, field, ctypes.POINTER(ctypes.c_float)())
        for code, msg in (_forward(d), _size(d)[::2]):
            assert code == _lib.THZ_E_ARG and "null" in msg


def test_shape_rules_of_the_planes():
    """thz_rsc_forward's rules from the one shared function: the same codes for the same shapes."""
    from quantizationawarethzdoe_amd import _lib

    def plane_code(d):
        p = _lib.RscDesc(B=d.B, C=d.C, H=d.H, W=d.W, vectorial=d.vectorial, dx=d.dx, dy=d.dy, z=0.02,
                         wavelengths=d.wavelengths, adjoint=0)
        n = ctypes.c_size_t(0)
        return _lib.lib().thz_rsc_workspace_size(ctypes.byref(p), ctypes.byref(n))

    for kw, want in ((dict(B=0), _lib.THZ_E_ARG), (dict(W=0), _lib.THZ_E_ARG), (dict(C=0), _lib.THZ_E_ARG),
                     (dict(vectorial=1, B=1), _lib.THZ_E_ARG), (dict(C=65), _lib.THZ_E_UNSUPPORTED),
                     (dict(H=8200, W=64), _lib.THZ_E_UNSUPPORTED), (dict(H=64, W=8194), _lib.THZ_E_UNSUPPORTED)):
        _, d = _desc(**kw)
        code, msg = _forward(d)
        assert code == want == _size(d)[0] == plane_code(d), (kw, code, msg)
        assert msg
    _, d = _desc(vectorial=1, B=2)
    assert _size(d)[0] == _lib.THZ_OK
    _, d = _desc(H=8192, W=8192, row=8191)
    assert _size(d)[0] == _lib.THZ_OK


def test_short_or_null_workspace():
    _lib, d = _desc()
    _, need, _ = _size(d)
    code, msg = _forward(d, ws_bytes=need - 1)
    assert code == _lib.THZ_E_WORKSPACE and str(need) in msg
    code, msg = _forward(d, ws=0)
    assert code == _lib.THZ_E_WORKSPACE and str(need) in msg


def _r256(n):
    return (n + 255) // 256 * 256


def _formula(B, C, H, W, Z, vectorial=False):
    """include/thzdoe.h: Uh + P."""
    Pw = W + 2 * (W // 2)
    Bo = 3 if vectorial else B
    zc = min(Z, 32)
    hs = max(1, min(H, 64, 2048 // (32 * C)))
    return _r256(8 * ((2 + zc) if vectorial else B) * C * H * Pw) + _r256(8 * zc * Bo * C * hs * Pw)


def test_workspace_holds_the_row_spectra_and_one_chunk_of_partial_sums():
    """1024 x 1024, C = 2, B = 1: the header's formula, below the workspace of ONE full plane (no
    Ph x Pw kernel table or spectrum), and no growth with Z past the library's chunk (32 planes)."""
    sizes = {}
    for Z in (1, 16, 32, 64, 200):
        _lib, d = _desc(Z=Z)
        code, n, _ = _size(d)
        assert code == _lib.THZ_OK
        sizes[Z] = n
        plane = _lib.RscDesc(B=1, C=2, H=1024, W=1024, vectorial=0, dx=d.dx, dy=d.dy, z=0.02,
                             wavelengths=d.wavelengths, adjoint=0)
        full = ctypes.c_size_t(0)
        assert _lib.lib().thz_rsc_workspace_size(ctypes.byref(plane), ctypes.byref(full)) == _lib.THZ_OK
        assert n < full.value, (Z, n, full.value)
        assert n == _formula(1, 2, 1024, 1024, Z), (Z, n)
    assert sizes[1] < sizes[16] < sizes[32] == sizes[64] == sizes[200]


@pytest.mark.parametrize("shape", [(2, 1, 33, 47, False), (2, 3, 40, 512, True), (4, 1, 16, 1024, False),
                                   (2, 2, 24, 8192, True), (1, 1, 2, 3, False)])
def test_workspace_formula_on_other_shapes(shape):
    B, C, H, W, vec = shape
    for Z in (1, 5, 40):
        _lib, d = _desc(H=H, W=W, C=C, B=B, Z=Z, row=0, vectorial=int(vec))
        code, n, msg = _size(d)
        assert code == _lib.THZ_OK, msg
        assert n == _formula(B, C, H, W, Z, vec), (shape, Z, n)


def test_propagate_zx_argument_errors_without_gpu():
    """row and axis are checked before anything touches a device; RSC_prop keeps its B == 1 rule."""
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    from quantizationawarethzdoe_amd.Props.RSC_Prop import RSC_prop, VRS_prop
    for cls, B in ((RSC_prop, 1), (VRS_prop, 2)):
        field = ElectricField(torch.ones(B, 1, 17, 12, dtype=torch.complex64), wavelengths=1e-3,
                              spacing=[1e-3, 1e-3], device="cpu")
        prop = cls(z_distance=0.1, device="cpu")
        with pytest.raises(ValueError, match=r"\[0, 16\)"):
            prop.propagate_zx(field, [0.1, 0.2], row=16)
        with pytest.raises(ValueError, match=r"\[0, 12\)"):
            prop.propagate_zx(field, [0.1, 0.2], row=-1, axis="y")
        with pytest.raises(ValueError, match=r"\[0, 12\)"):
            prop.propagate_zx(field, [0.1, 0.2], row=12, axis="y")
        with pytest.raises(ValueError, match="'x' or 'y'"):
            prop.propagate_zx(field, [0.1, 0.2], axis="z")
        one = ElectricField(torch.ones(B, 1, 1, 12, dtype=torch.complex64), wavelengths=1e-3, spacing=[1e-3, 1e-3],
                            device="cpu")
        with pytest.raises(ValueError, match=r"\[0, 0\)"):
            prop.propagate_zx(one, [0.1])
    two = ElectricField(torch.ones(2, 1, 16, 12, dtype=torch.complex64), wavelengths=1e-3, spacing=[1e-3, 1e-3],
                        device="cpu")
    with pytest.raises(RuntimeError, match="B == 1"):
        RSC_prop(z_distance=0.1, device="cpu").propagate_zx(two, [0.1])
    with pytest.raises(RuntimeError, match="B == 1"):
        RSC_prop(z_distance=0.1, device="cpu").propagate_planes(two, [0.1])


# ---------------------------------------------------------------------------------------------
# The identity the kernels implement, restated in torch (fp64) and held against the oracle
# ---------------------------------------------------------------------------------------------
def slice_identity(data, lam, dx, dy, z, p):
    """Row p of rsc_forward's [B, C, Ho, Wo] plane as a sum over the H input rows of 1-D circular
    convolutions of length Pw: dx dy IFFT(sum_i FFT(in[i] padded) FFT(RS(x[H + p - i], y)))[W:]."""
    B, C, H, W = data.shape
    Ph, Pw = H + 2 * (H // 2), W + 2 * (W // 2)
    x = torch.linspace(-Ph * dx / 2, Ph * dx / 2, Ph)
    y = torch.linspace(-Pw * dx / 2, Pw * dx / 2, Pw)
    a = H + p - torch.arange(H)                                         # the kernel rows: never wraps
    assert int(a.min()) >= 1 and int(a.max()) <= Ph - 1
    k = 2 * torch.pi / lam[:, None, None]
    r = torch.sqrt(x[a][None, :, None] ** 2 + y[None, None, :] ** 2 + z ** 2)     # [1, H, Pw]
    K = torch.exp(1j * k * r) * (1 / (2 * torch.pi) * z / r ** 2 * (1 / r - 1j * k))   # [C, H, Pw]
    Uh = torch.fft.fft(data, n=Pw, dim=-1)                               # [B, C, H, Pw]
    S = (Uh * torch.fft.fft(K, dim=-1)[None]).sum(-2)
    return torch.fft.ifft(S, dim=-1)[..., W:] * dx * dy


def vrs_planes(data, dx, z):
    """[Ex, Ey, Ez] with Ez = Ex x / r + Ey y / r on the unpadded grid (dx on both axes), as
    _RscFunction's docstring and Props/RSC_Prop.py:294-303 form it."""
    H, W = data.shape[-2:]
    xs = torch.linspace(-H * dx / 2, H * dx / 2, H)
    ys = torch.linspace(-W * dx / 2, W * dx / 2, W)
    X, Y = torch.meshgrid(xs, ys, indexing="ij")
    r = torch.sqrt(X ** 2 + Y ** 2 + z ** 2)
    return torch.cat([data[0:1], data[1:2], data[0:1] * X / r + data[1:2] * Y / r], 0)


def _rows(Ho):
    return sorted({0, Ho // 2, Ho - 1})


@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: f"{g[0]}x{g[1]}")
def test_identity_equals_the_oracle_planes_fp64(geo):
    from oracle import thz_oracle as orc
    H, W, C, B, (dx, dy) = geo
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        g = torch.Generator().manual_seed(H * 1000 + W)
        data = torch.randn(B, C, H, W, dtype=torch.complex128, generator=g)
        lam = torch.tensor([1e-3 * (1 + 0.1 * c) for c in range(C)])
        for z in ZS:
            ref = torch.cat([orc.rsc_forward(data[b:b + 1], lam, [dx, dy], z) for b in range(B)], 0)
            for p in _rows(2 * (H // 2)):
                got, want = slice_identity(data, lam, dx, dy, z, p), ref[:, :, p, :]
                rel = float((got - want).norm() / want.norm())
                assert rel <= 1e-12, (geo, z, p, rel)
            # axis="y": column q of the planes is row q of the transposed field's planes, same spacing
            for q in _rows(2 * (W // 2)):
                got = slice_identity(data.transpose(-1, -2).contiguous(), lam, dx, dy, z, q)
                want = ref[:, :, :, q]
                rel = float((got - want).norm() / want.norm())
                assert rel <= 1e-12, (geo, z, q, rel)
    finally:
        torch.set_default_dtype(old)


def test_identity_vrs_and_its_transposition_rule_fp64():
    """VRS 40 x 48, dx != dy: the three planes by the identity (Ez formed per z), and axis="y" as the
    transposed field with Ex / Ey exchanged going in and planes 0 / 1 exchanged coming out."""
    from oracle import thz_oracle as orc
    H, W, dx, dy = 40, 48, 1e-3, 1.2e-3
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        g = torch.Generator().manual_seed(9)
        data = torch.randn(2, 2, H, W, dtype=torch.complex128, generator=g)
        lam = torch.tensor([1e-3, 1.1e-3])
        for z in ZS:
            vec = vrs_planes(data, dx, z)
            ref = torch.cat([orc.rsc_forward(vec[b:b + 1], lam, [dx, dy], z) for b in range(3)], 0)
            for p in _rows(H):
                got, want = slice_identity(vec, lam, dx, dy, z, p), ref[:, :, p, :]
                assert float((got - want).norm() / want.norm()) <= 1e-12, (z, p)
            swapped = vrs_planes(data.transpose(-1, -2)[[1, 0]].contiguous(), dx, z)
            for q in _rows(W):
                got = slice_identity(swapped, lam, dx, dy, z, q)[[1, 0, 2]]
                want = ref[:, :, :, q]
                assert float((got - want).norm() / want.norm()) <= 1e-12, (z, q)
    finally:
        torch.set_default_dtype(old)
