"""The adjoint entries of the RSC / VRS z-x slice (thz_rsc_slice_adjoint_workspace_size,
thz_rsc_slice_adjoint; ABI 9, additive) without a GPU: the symbols are exported and bound, every
validation path returns the forward's code and message before any device call, the workspace is the
header's formula (S and one chunk of cotangent lines, nothing of a plane's size), ``grad`` is validated
on a CPU field, and the three-step adjoint the kernels implement -- cotangent lines transformed, the
kernel rows' conjugated spectra summed over the planes in the spectrum, one inverse transform per input
row; VRS's third plane inverted per plane for its x/r, y/r factors -- written out in torch fp64 with no
autograd equals autograd through the oracle's planes.
"""
import ctypes

import pytest
import torch

from oracle import thz_oracle as orc


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


def _adjoint(d, gout=8, gin=8, ws=8, ws_bytes=1 << 40):
    """The data pointers are never dereferenced: every call here fails its validation first."""
    from quantizationawarethzdoe_amd import _lib
    code = _lib.lib().thz_rsc_slice_adjoint(ctypes.byref(d), ctypes.c_void_p(gout), ctypes.c_void_p(gin),
                                            ctypes.c_void_p(ws), ctypes.c_size_t(ws_bytes), None)
    return code, _lib.lib().thz_last_error().decode()


def _size(d, forward=False):
    from quantizationawarethzdoe_amd import _lib
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    fn = L.thz_rsc_slice_workspace_size if forward else L.thz_rsc_slice_adjoint_workspace_size
    code = fn(ctypes.byref(d), ctypes.byref(n))
    return code, n.value, L.thz_last_error().decode()


def test_symbols_exported_bound_and_abi_9():
    from quantizationawarethzdoe_amd import _lib
    h = _lib.lib()
    names = {"thz_rsc_slice_adjoint_workspace_size", "thz_rsc_slice_adjoint"}
    assert all(hasattr(h, n) for n in names) and names <= set(_lib.EXPORTED)
    assert len(h.thz_rsc_slice_adjoint.argtypes) == 6
    assert len(h.thz_rsc_slice_adjoint_workspace_size.argtypes) == 2
    assert h.thz_abi_version() == 9 == _lib.THZ_ABI_VERSION


def test_null_descriptor_bytes_data_z_and_wavelengths():
    from quantizationawarethzdoe_amd import _lib
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    assert L.thz_rsc_slice_adjoint_workspace_size(None, ctypes.byref(n)) == _lib.THZ_E_ARG
    assert b"null" in L.thz_last_error()
    _, d = _desc()
    assert L.thz_rsc_slice_adjoint_workspace_size(ctypes.byref(d), None) == _lib.THZ_E_ARG
    assert b"null" in L.thz_last_error()
    assert L.thz_rsc_slice_adjoint(None, ctypes.c_void_p(8), ctypes.c_void_p(8), ctypes.c_void_p(8),
                                   ctypes.c_size_t(1 << 40), None) == _lib.THZ_E_ARG
    assert b"null" in L.thz_last_error()
    for null in ("gout", "gin"):
        code, msg = _adjoint(d, **{null: 0})
        assert code == _lib.THZ_E_ARG and "null" in msg
    for field in ("z", "wavelengths"):
        _, d = _desc()
        setattr(d, field, ctypes.POINTER(ctypes.c_float)())
        for code, msg in (_adjoint(d), _size(d)[::2]):
            assert code == _lib.THZ_E_ARG and "null" in msg


@pytest.mark.parametrize("row", [-1, 1024, 1 << 20])
def test_bad_row_names_the_valid_range(row):
    """Ph - H = 1024 output rows at H = 1024."""
    _lib, d = _desc(row=row)
    for code, msg in (_adjoint(d), _size(d)[::2]):
        assert code == _lib.THZ_E_ARG and "row" in msg and "[0, 1024)" in msg


@pytest.mark.parametrize("Z", [0, 257])
def test_plane_count_outside_1_to_max_z(Z):
    _lib, d = _desc()
    assert _lib.THZ_MAX_Z == 256
    d.Z = Z
    for code, msg in (_adjoint(d), _size(d)[::2]):
        assert code == _lib.THZ_E_ARG and "Z=" in msg and "256" in msg


def test_shape_rules_are_the_forwards():
    from quantizationawarethzdoe_amd import _lib
    for kw, want in ((dict(vectorial=1, B=1), _lib.THZ_E_ARG), (dict(C=_lib.THZ_MAX_WAVELENGTHS + 1),
                                                               _lib.THZ_E_UNSUPPORTED),
                     (dict(B=0), _lib.THZ_E_ARG), (dict(H=64, W=8194), _lib.THZ_E_UNSUPPORTED)):
        _, d = _desc(**kw)
        code, msg = _adjoint(d)
        fcode, _, fmsg = _size(d, forward=True)
        assert code == want == _size(d)[0] == fcode, (kw, code, msg)
        assert msg == fmsg, "one validation function: the forward's messages"
    _, d = _desc(vectorial=1, B=2)
    assert _size(d)[0] == _lib.THZ_OK


def test_short_or_null_workspace_names_the_size():
    _lib, d = _desc()
    _, need, _ = _size(d)
    code, msg = _adjoint(d, ws_bytes=need - 1)
    assert code == _lib.THZ_E_WORKSPACE and str(need) in msg
    code, msg = _adjoint(d, ws=0)
    assert code == _lib.THZ_E_WORKSPACE and str(need) in msg


def _r256(n):
    return (n + 255) // 256 * 256


def _formula(B, C, H, W, Z, vectorial=False):
    """include/thzdoe.h: S + Gh."""
    Pw = W + 2 * (W // 2)
    Bo = 3 if vectorial else B
    zc = min(Z, 32)
    return _r256(8 * ((2 + zc) if vectorial else B) * C * H * Pw) + _r256(8 * zc * Bo * C * Pw)


def test_workspace_is_the_headers_formula():
    """1024 x 1024, C = 2, B = 1: S and one chunk of cotangent lines; no growth with Z past the library's
    chunk (32 planes); below the workspace of ONE full plane (no Ph x Pw kernel table or spectrum)."""
    sizes = {}
    for Z in (1, 32, 256):
        _lib, d = _desc(Z=Z)
        code, n, _ = _size(d)
        assert code == _lib.THZ_OK and n == _formula(1, 2, 1024, 1024, Z), (Z, n)
        sizes[Z] = n
    assert sizes[1] < sizes[32] == sizes[256]
    plane = _lib.RscDesc(B=1, C=2, H=1024, W=1024, vectorial=0, dx=d.dx, dy=d.dy, z=0.02,
                         wavelengths=d.wavelengths, adjoint=0)
    full = ctypes.c_size_t(0)
    assert _lib.lib().thz_rsc_workspace_size(ctypes.byref(plane), ctypes.byref(full)) == _lib.THZ_OK
    assert sizes[256] < full.value, (sizes[256], full.value)


@pytest.mark.parametrize("shape", [(2, 1, 33, 47, False), (2, 3, 40, 512, True), (4, 1, 16, 1024, False),
                                   (2, 2, 24, 8192, True), (1, 1, 2, 3, False)])
def test_workspace_formula_on_other_shapes(shape):
    B, C, H, W, vec = shape
    for Z in (1, 5, 40):
        _lib, d = _desc(H=H, W=W, C=C, B=B, Z=Z, row=0, vectorial=int(vec))
        code, n, msg = _size(d)
        assert code == _lib.THZ_OK, msg
        assert n == _formula(B, C, H, W, Z, vec), (shape, Z, n)


def test_grad_keyword_is_validated_without_gpu():
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    from quantizationawarethzdoe_amd.Props.RSC_Prop import RSC_prop, VRS_prop
    for cls, B in ((RSC_prop, 1), (VRS_prop, 2)):
        field = ElectricField(torch.ones(B, 1, 16, 12, dtype=torch.complex64), wavelengths=1e-3,
                              spacing=[1e-3, 1e-3], device="cpu")
        prop = cls(z_distance=0.1, device="cpu")
        with pytest.raises(ValueError, match="grad must be 'planes' or 'slice', got 'rows'"):
            prop.propagate_zx(field, [0.1, 0.2], grad="rows")


# ----------------------------------------------------------------------------------------------
# the decomposition in fp64
# ----------------------------------------------------------------------------------------------
# (H, W, C, (dx, dy), vectorial, planes)
CASES = [
    (72, 100, 2, (0.25e-3, 0.3e-3), False, (0.030, 0.0725)),
    (33, 47, 1, (0.25e-3, 0.25e-3), False, (0.030, 0.041, 0.0725)),
    (20, 24, 1, (0.5e-3, 0.5e-3), False, (0.030, 0.041, 0.0725)),
    (40, 48, 2, (0.25e-3, 0.3e-3), True, (0.030, 0.041, 0.0725)),
]


def _lam(C):
    return torch.tensor([1e-3 * (1 + 0.1 * c) for c in range(C)])


def _ez_factors(H, W, dx, z):
    xs = torch.linspace(-H * dx / 2, H * dx / 2, H)
    ys = torch.linspace(-W * dx / 2, W * dx / 2, W)
    X, Y = torch.meshgrid(xs, ys, indexing="ij")
    rr = torch.sqrt(X ** 2 + Y ** 2 + z ** 2)
    return X / rr, Y / rr


def _three_step_adjoint(g, H, W, C, dx, dy, zs, row, vectorial):
    """grad_in [B, C, H, W] of the cotangent g [Z, Bo, C, Wo], by the three steps of DESIGN.md section 20."""
    Ph, Pw = H + 2 * (H // 2), W + 2 * (W // 2)
    Z, Bo = g.shape[:2]
    lam = _lam(C)
    kw = 2 * torch.pi / lam[:, None, None]
    x = torch.linspace(-Ph * dx / 2, Ph * dx / 2, Ph)
    y = torch.linspace(-Pw * dx / 2, Pw * dx / 2, Pw)
    a = H + row - torch.arange(H)   # the kernel row each input row meets
    mx, my = torch.meshgrid(x[a], y, indexing="ij")
    scale = dx * dy / Pw
    # 1. the cotangent lines
    pad = torch.zeros(Z, Bo, C, Pw, dtype=torch.complex128)
    pad[..., W:] = g
    Gh = scale * torch.fft.fft(pad, dim=-1)
    # 2. the planes summed in the spectrum (VRS's third plane kept per plane)
    nsum = 2 if vectorial else Bo
    S = torch.zeros(nsum, C, H, Pw, dtype=torch.complex128)
    gin = torch.zeros(nsum, C, H, W, dtype=torch.complex128)
    for k, z in enumerate(zs):
        r = torch.sqrt(mx ** 2 + my ** 2 + z ** 2)
        K = torch.exp(1j * kw * r) * (1 / (2 * torch.pi) * z / r ** 2 * (1 / r - 1j * kw))   # [C, H, Pw]
        Kh = torch.fft.fft(K, dim=-1)
        S += Kh.conj()[None] * Gh[k, :nsum, :, None, :]
        if vectorial:
            e = torch.fft.ifft(Kh.conj() * Gh[k, 2, :, None, :], dim=-1)[..., :W] * Pw
            fx, fy = _ez_factors(H, W, dx, z)
            gin[0] += fx * e
            gin[1] += fy * e
    # 3. one unnormalised inverse transform per input row
    return gin + torch.fft.ifft(S, dim=-1)[..., :W] * Pw


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}x{c[1]}{'vrs' if c[4] else ''}")
def test_three_step_adjoint_equals_autograd_through_the_oracle(case):
    H, W, C, (dx, dy), vectorial, zs = case
    Ho, Wo = 2 * (H // 2), 2 * (W // 2)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        gen = torch.Generator().manual_seed(1000 * H + W)
        B = 2 if vectorial else 1
        x = torch.randn(B, C, H, W, dtype=torch.complex128, generator=gen).requires_grad_(True)
        planes = []
        for z in zs:
            v = x
            if vectorial:
                fx, fy = _ez_factors(H, W, dx, z)
                v = torch.cat([x[0:1], x[1:2], x[0:1] * fx + x[1:2] * fy], 0)
            planes.append(torch.cat([orc.rsc_forward(v[b:b + 1], _lam(C), [dx, dy], z) for b in range(v.shape[0])], 0))
        planes = torch.stack(planes)   # [Z, Bo, C, Ho, Wo]
        for row in (0, Ho // 2, Ho - 1):
            g = torch.randn(len(zs), planes.shape[1], C, Wo, dtype=torch.complex128, generator=gen)
            want, = torch.autograd.grad(planes[..., row, :], x, grad_outputs=g, retain_graph=True)
            with torch.no_grad():
                got = _three_step_adjoint(g, H, W, C, dx, dy, zs, row, vectorial)
            err = float((got - want).norm() / want.norm())
            print(f"three-step adjoint {H}x{W} vec {vectorial} row {row}: vs autograd {err:.3e}")
            assert err <= 1e-12, (row, err)
    finally:
        torch.set_default_dtype(old)
