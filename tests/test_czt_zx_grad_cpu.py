"""The adjoint entries of the CZT z-x slice (thz_czt_slice_adjoint_workspace_size,
thz_czt_slice_adjoint; ABI 9, additive) and propagate_zx(grad=...) without a GPU: the symbols are
exported, every validation path returns its code before any device call, the workspace holds one
chunk's tables and T only, and the two-step adjoint the kernels implement (line adjoint, expand),
written out explicitly in torch fp64, equals autograd through the oracle's planes.
"""
import ctypes
import math

import pytest
import torch

# (H, W, out, C, B, (dx, dy), (odx, ody)): the geometries of tests/test_czt_zx_cpu.py
GEOMETRIES = [
    (72, 100, 40, 2, 2, (0.25e-3, 0.3e-3), (0.1e-3, 0.12e-3)),
    (48, 48, 64, 1, 1, (0.25e-3, 0.25e-3), (0.05e-3, 0.05e-3)),
    (130, 70, 33, 3, 1, (0.25e-3, 0.25e-3), (0.1e-3, 0.1e-3)),
    (20, 24, 20, 1, 2, (0.5e-3, 0.5e-3), (0.2e-3, 0.2e-3)),
]
NAMES = {"thz_czt_slice_adjoint_workspace_size", "thz_czt_slice_adjoint"}


def _desc(H=2048, W=2048, out=512, C=2, B=1, Z=3, row=5, **kw):
    from quantizationawarethzdoe_amd import _lib, propagation as P
    d = P._czt_slice_desc(B, C, H, W, out, out, (0.25e-3, 0.25e-3), 0.05e-3, 0.05e-3,
                          [1e-3 * (1 + 0.1 * c) for c in range(C)], [0.02 + 0.001 * k for k in range(Z)], row)
    for k, v in kw.items():
        setattr(d, k, v)
    return _lib, d


def _adjoint(d, g=8, gin=8, ws=8, ws_bytes=1 << 40):
    from quantizationawarethzdoe_amd import _lib
    code = _lib.lib().thz_czt_slice_adjoint(ctypes.byref(d), ctypes.c_void_p(g), ctypes.c_void_p(gin),
                                            ctypes.c_void_p(ws), ctypes.c_size_t(ws_bytes), None)
    return code, _lib.lib().thz_last_error().decode()


def _size(d):
    from quantizationawarethzdoe_amd import _lib
    n = ctypes.c_size_t(0)
    code = _lib.lib().thz_czt_slice_adjoint_workspace_size(ctypes.byref(d), ctypes.byref(n))
    return code, n.value, _lib.lib().thz_last_error().decode()


def test_symbols_exported_bound_and_abi_still_9():
    from quantizationawarethzdoe_amd import _lib
    h = _lib.lib()
    assert all(hasattr(h, n) for n in NAMES) and NAMES <= set(_lib.EXPORTED)
    assert h.thz_czt_slice_adjoint.argtypes is not None and len(h.thz_czt_slice_adjoint.argtypes) == 6
    assert h.thz_abi_version() == 9 == _lib.THZ_ABI_VERSION


def test_null_descriptor_bytes_and_data():
    from quantizationawarethzdoe_amd import _lib
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    assert L.thz_czt_slice_adjoint_workspace_size(None, ctypes.byref(n)) == _lib.THZ_E_ARG
    assert b"null" in L.thz_last_error()
    _, d = _desc()
    assert L.thz_czt_slice_adjoint_workspace_size(ctypes.byref(d), None) == _lib.THZ_E_ARG
    assert b"null" in L.thz_last_error()
    assert L.thz_czt_slice_adjoint(None, ctypes.c_void_p(8), ctypes.c_void_p(8), ctypes.c_void_p(8),
                                   ctypes.c_size_t(1 << 40), None) == _lib.THZ_E_ARG
    assert b"null" in L.thz_last_error()
    for null in ("g", "gin"):
        code, msg = _adjoint(d, **{null: 0})
        assert code == _lib.THZ_E_ARG and "null" in msg
    for field in ("z", "wavelengths"):
        _, d = _desc()
        setattr(d, field, ctypes.POINTER(ctypes.c_float)())
        code, msg = _adjoint(d)
        assert code == _lib.THZ_E_ARG and "null" in msg


@pytest.mark.parametrize("row", [-1, 512, 1 << 20])
def test_bad_row_is_an_argument_error(row):
    _lib, d = _desc(row=row)
    for code, msg in (_adjoint(d), _size(d)[::2]):
        assert code == _lib.THZ_E_ARG and "row" in msg and "[0, 512)" in msg


@pytest.mark.parametrize("Z", [0, 257])
def test_plane_count_outside_1_to_max_z(Z):
    _lib, d = _desc()
    assert _lib.THZ_MAX_Z + 1 == 257
    d.Z = Z
    for code, msg in (_adjoint(d), _size(d)[::2]):
        assert code == _lib.THZ_E_ARG and "Z=" in msg and "256" in msg


def test_shape_rules_of_the_forward():
    _lib, d = _desc()
    d.outW = 500
    for code, msg in (_adjoint(d), _size(d)[::2]):
        assert code == _lib.THZ_E_ARG and "square" in msg
    _lib, d = _desc(H=33, W=33, out=32, row=0)   # m + M - 1 = 64
    for code, msg in (_adjoint(d), _size(d)[::2]):
        assert code == _lib.THZ_E_ARG and "power of two" in msg and "64" in msg
    _lib, d = _desc(H=16000, W=16000, out=512)   # np2 = 32768
    code, msg = _adjoint(d)
    assert code == _lib.THZ_E_UNSUPPORTED and "16384" in msg


def test_short_or_null_workspace():
    _lib, d = _desc()
    _, need, _ = _size(d)
    code, msg = _adjoint(d, ws_bytes=need - 1)
    assert code == _lib.THZ_E_WORKSPACE and str(need) in msg
    code, msg = _adjoint(d, ws=0)
    assert code == _lib.THZ_E_WORKSPACE and str(need) in msg


def test_workspace_is_one_chunk_of_tables_and_t():
    """(2048, 2048) -> 512, C = 2, B = 1: the header's formula, no growth past one 16-plane chunk,
    below the workspace of one full plane."""
    def a256(n):
        return (n + 255) // 256 * 256

    sizes = {}
    for Z in (16, 256):
        _lib, d = _desc(Z=Z)
        code, n, _ = _size(d)
        assert code == _lib.THZ_OK
        sizes[Z] = n
    zc, C, B, H, W, out, np2 = 16, 2, 1, 2048, 2048, 512, 4096
    assert sizes[16] == a256(8 * zc * C * (W + out + np2 + H + 32)) + a256(8 * zc * B * C * W)
    assert sizes[16] == sizes[256]
    plane = _lib.CztDesc(B=B, C=C, H=H, W=W, outH=out, outW=out, dx=d.dx, dy=d.dy, odx=d.odx, ody=d.ody,
                         z=0.02, wavelengths=d.wavelengths, adjoint=1)
    full = ctypes.c_size_t(0)
    assert _lib.lib().thz_czt_workspace_size(ctypes.byref(plane), ctypes.byref(full)) == _lib.THZ_OK
    assert sizes[256] < full.value


def test_grad_keyword_is_validated_without_gpu():
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    from quantizationawarethzdoe_amd.Props.CZT_Prop import CZT_prop, VCZT_prop
    field = ElectricField(torch.ones(1, 1, 16, 12, dtype=torch.complex64), wavelengths=1e-3, spacing=[1e-3, 1e-3],
                          device="cpu")
    for cls in (CZT_prop, VCZT_prop):
        prop = cls(z_distance=0.1, device="cpu")
        with pytest.raises(ValueError, match="grad must be 'planes' or 'slice', got 'rows'"):
            prop.propagate_zx(field, [0.1, 0.2], grad="rows")


# ---------------------------------------------------------------------------------------------
# The adjoint the kernels implement, written out step by step in torch fp64 (no autograd here)
# ---------------------------------------------------------------------------------------------
def _pass_tables(lam, z, dx, m, M, lo, hi):
    """thA, thW, D1, D2, Dm [C, 1] of one Bluestein pass (czt_tables / czt_slice_tables)."""
    Dm = (lam * z / dx).reshape(-1, 1)
    f1, f2 = lo + Dm / 2, hi + Dm / 2
    D1 = f1 + (M * Dm + f2 - f1) / (2 * M)
    D2 = f2 + (M * Dm + f2 - f1) / (2 * M)
    return 2 * math.pi * D1 / Dm, -2 * math.pi * (D1 - D2) / (M * Dm), D1, D2, Dm


def _post(thW, D1, D2, Dm, m, M, l):
    ell = l / M * (D2 - D1) + D1
    return torch.exp(1j * (thW * l * l / 2 - 2 * math.pi * ell * (-m / 2 + 0.5) / Dm))


def slice_adjoint(g, lam, spacing, z, out, odx, ody, p, H, W):
    """A_{z,p}^H g for g [B, C, outH]: step 1 (line adjoint) -> T [B, C, W], step 2 (expand) ->
    [B, C, H, W].  Also tells whether coef met its ntab cut."""
    from oracle import thz_oracle as orc
    dx, dy = spacing
    C, M = lam.numel(), out
    xi = torch.linspace(-H * dx / 2, H * dx / 2, H)
    yi = torch.linspace(-W * dy / 2, W * dy / 2, W)
    imx, imy = torch.meshgrid(xi, yi, indexing="ij")
    xo = torch.linspace(-out * odx / 2, out * odx / 2, out)
    yo = torch.linspace(-out * ody / 2, out * ody / 2, out)
    zero = torch.zeros((), dtype=torch.complex128)
    # pass B (H axis, fy, M = outW): coef[h] = preB[h] gB[p + H - h], postB[p] without 1/nrm
    thA, thW, D1, D2, Dm = _pass_tables(lam, z, dx, H, M, yo[0], yo[-1])
    h = torch.arange(H, dtype=torch.float64)[None, :]
    t = p + H - h
    ntabB = min(H + M, H + max(M - 1, H - 1))
    coef = torch.exp(1j * (-thA * h + thW * h * h / 2)) * torch.where(
        t < ntabB, torch.exp(-1j * thW * (t - H + 1) ** 2 / 2), zero)          # [C, H]
    postB = _post(thW, D1, D2, Dm, H, M, float(p))                              # [C, 1]
    # pass A (W axis, fx, M = outH): pre, post, filter spectrum of 1/h (zero from ntab on)
    thA, thW, D1, D2, Dm = _pass_tables(lam, z, dx, W, M, xo[0], xo[-1])
    m, mp = W, W + M - 1
    N = 2 ** int(math.ceil(math.log2(mp)))
    w = torch.arange(m, dtype=torch.float64)[None, :]
    q = torch.arange(M, dtype=torch.float64)[None, :]
    preA = torch.exp(1j * (-thA * w + thW * w * w / 2))                         # [C, W]
    postA = _post(thW, D1, D2, Dm, m, M, q)                                     # [C, outH]
    n = torch.arange(N, dtype=torch.float64)[None, :]
    ntabA = min(mp + 1, m + max(M - 1, m - 1))
    ft = torch.fft.fft(torch.where(n < ntabA, torch.exp(-1j * thW * (n - m + 1) ** 2 / 2), zero), dim=-1)
    F0 = orc._rs_kernel(z, xo[p].expand(1, out), yo[None, :], lam)[0]           # [C, 1, outH]
    cst = (z * odx * ody * lam).reshape(C, 1)
    # step 1: Z[(q + m) mod N] = conj(postA[q]) conj(cst F0 postB) g[q]; T = conj(preA) IFFT(FFT(Z) conj(ft))[:W]
    Z = torch.zeros(g.shape[0], C, N, dtype=torch.complex128)
    Z[..., (torch.arange(M) + m) % N] = (postA * cst * F0[:, 0, :] * postB).conj() * g
    T = preA.conj() * torch.fft.ifft(torch.fft.fft(Z, dim=-1) * ft.conj(), dim=-1)[..., :m]
    # step 2: gin[b,c,h,w] = conj(F(x_h, y_w)) conj(coef[h]) T[b,c,w]
    F = orc._rs_kernel(z, imx, imy, lam)                                         # [1, C, H, W]
    return F.conj() * coef.conj()[None, :, :, None] * T[:, :, None, :], bool((t >= ntabB).any())


@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: f"{g[0]}x{g[1]}to{g[2]}")
def test_adjoint_decomposition_equals_autograd_through_the_oracle_fp64(geo):
    from oracle import thz_oracle as orc
    H, W, out, C, B, spacing, (odx, ody) = geo
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        gen = torch.Generator().manual_seed(H * 1000 + W)
        data = torch.randn(B, C, H, W, dtype=torch.complex128, generator=gen).requires_grad_(True)
        lam = torch.tensor([1e-3 * (1 + 0.1 * c) for c in range(C)])
        hit_ntab = False
        for z in (0.03, 0.07):
            planes = orc.czt_forward(data, lam, list(spacing), z, out, out, odx, ody)
            for p in (0, out // 2, out - 1):
                g = torch.randn(B, C, out, dtype=torch.complex128, generator=gen)
                want, = torch.autograd.grad(planes[:, :, p, :], data, grad_outputs=g, retain_graph=True)
                got, cut = slice_adjoint(g, lam, spacing, z, out, odx, ody, p, H, W)
                hit_ntab |= cut
                rel = float((got - want).norm() / want.norm())
                assert rel <= 1e-12, (geo, z, p, rel)
        assert hit_ntab == (out >= H)
    finally:
        torch.set_default_dtype(old)
