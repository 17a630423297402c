"""The native backward of the CZT z-x slice on the GPU: CZT_prop.propagate_zx(..., grad="slice") runs the
slice kernels forward (czt_slice_collapse / czt_slice_line) and their adjoint backward
(thz_czt_slice_adjoint: czt_slice_line_adj on the cotangent rows, czt_slice_expand), so a loss on the
zoomed axial map never forms a plane.

Geometries, sweep and inputs as tests/test_czt_zx_gpu.py; cotangents are seeded white complex noise.

Bounds:
* adjoint identity against the native forward: |<A x, g> - <x, A^H g>| <= 1e-5 ||A x|| ||g||, the dot
  products in complex128 (the bound of tests/test_properties_gpu.py and tests/test_asm_zx_grad_gpu.py);
* against autograd through the fp64 oracle on the fp32-rounded parameters: rel-L2 <= 1e-3, the
  project's CZT bound (tests/test_czt_gpu.py);
* against the full-plane adjoint (the cotangent at row p of zero planes through
  czt_apply(adjoint=True), summed over the planes) and between the two ``grad`` forms: <= 2e-3, the
  triangle inequality of two results each within 1e-3 of the oracle;
* complex128 (the fp64 planes serve it): <= 1e-8, the project's fp64 CZT bound (tests/test_f64_gpu.py).
"""
import functools

import pytest
import torch

from oracle import thz_oracle as orc

pytestmark = pytest.mark.gpu

# (H, W, out, C, B, (dx, dy), (odx, ody)): tests/test_czt_zx_gpu.py
GEOMETRIES = [
    (72, 100, 40, 2, 2, (0.25e-3, 0.3e-3), (0.1e-3, 0.12e-3)),
    (48, 48, 64, 1, 1, (0.25e-3, 0.25e-3), (0.05e-3, 0.05e-3)),
    (130, 70, 33, 3, 1, (0.25e-3, 0.25e-3), (0.1e-3, 0.1e-3)),
    (20, 24, 20, 1, 2, (0.5e-3, 0.5e-3), (0.2e-3, 0.2e-3)),
]
BIG = (1024, 1024, 256, 1, 1, (0.25e-3, 0.25e-3), (0.25e-3, 0.25e-3))   # np2 = 2048: the compile-time plan
ZS = (0.030, 0.041, 0.055, 0.0725, 0.090)
ORACLE_TOL, PLANES_TOL, IDENTITY_TOL, F64_TOL = 1e-3, 2e-3, 1e-5, 1e-8
IDS = dict(ids=lambda g: f"{g[0]}x{g[1]}to{g[2]}")


def _dev():
    return torch.device("cuda:0")


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def _lam(C):
    return [1e-3 * (1 + 0.1 * c) for c in range(C)]


def _rows(out):
    return (0, out // 2, out - 1)


@functools.lru_cache(maxsize=None)
def _input(geo, dtype=torch.complex64):
    H, W, out, C, B = geo[:5]
    g = torch.Generator().manual_seed(1000 * H + W)
    return torch.randn(B, C, H, W, dtype=torch.complex128, generator=g).to(dtype)


@functools.lru_cache(maxsize=None)
def _cotangent(geo, Z, row, dtype=torch.complex64):
    """Seeded white cotangent [Z, B, C, out] (never modified)."""
    H, W, out, C, B = geo[:5]
    g = torch.Generator().manual_seed(7919 * H + 31 * W + row)
    return torch.randn(Z, B, C, out, dtype=torch.complex128, generator=g).to(dtype)


def _field(geo, dtype=torch.complex64, grad=False, data=None):
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    C, spacing = geo[3], geo[5]
    if data is None:
        data = _input(geo, dtype).to(_dev())
        if grad:
            data.requires_grad_(True)
    wl = _lam(C)
    if dtype == torch.complex128:
        wl = torch.tensor(wl, dtype=torch.float64)
    elif C == 1:
        wl = wl[0]
    return ElectricField(data, wavelengths=wl, spacing=list(spacing), device=_dev())


def _prop(cls=None):
    from quantizationawarethzdoe_amd.Props.CZT_Prop import CZT_prop
    return (cls or CZT_prop)(z_distance=0.05, device=_dev())


def _grid(geo):
    out, (odx, ody) = geo[2], geo[6]
    return dict(outputHeight=out, outputWidth=out, outputPixel_dx=odx, outputPixel_dy=ody)


def _cfg(geo):
    """(wavelengths, spacing, out, out, odx, ody) as the kernels receive them."""
    H, W, out, C, B, spacing, (odx, ody) = geo
    return _lam(C), (_f32(spacing[0]), _f32(spacing[1])), out, out, odx, ody


@functools.lru_cache(maxsize=None)
def _oracle_grads(geo, zs, rows, exact=False):
    """{row: A_row^H g_row} [B, C, H, W] complex128 by autograd through the fp64 oracle's planes, one
    oracle forward per z shared by the rows; computed once and never modified.  The oracle sees the
    values the kernels are given: fp32 roundings, or with ``exact`` (complex128) the doubles
    themselves except the input spacing, which ElectricField stores as float32."""
    H, W, out, C, B, spacing, (odx, ody) = geo
    spacing = [_f32(spacing[0]), _f32(spacing[1])]
    r = (lambda v: v) if exact else _f32
    dt = torch.complex128 if exact else torch.complex64
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        x = _input(geo, dt).to(torch.complex128).requires_grad_(True)
        lam = torch.tensor([r(v) for v in _lam(C)])
        acc = {p: torch.zeros(B, C, H, W, dtype=torch.complex128) for p in rows}
        for k, z in enumerate(zs):
            planes = orc.czt_forward(x, lam, spacing, r(z), out, out, r(odx), r(ody))
            for p in rows:
                g = _cotangent(geo, len(zs), p, dt)[k].to(torch.complex128)
                acc[p] += torch.autograd.grad(planes[:, :, p, :], x, grad_outputs=g, retain_graph=True)[0]
        return acc
    finally:
        torch.set_default_dtype(old)


def _rel(got, want):
    got, want = got.to(torch.complex128).cpu(), want.to(torch.complex128).cpu()
    return float((got - want).norm() / want.norm())


def _dot(a, b):
    return complex(torch.vdot(a.reshape(-1).to(torch.complex128), b.reshape(-1).to(torch.complex128)))


def _launches(fn, name="czt_slice_expand"):
    """(result, launches of the expand kernel) of fn(): whether the native backward served the call."""
    from quantizationawarethzdoe_amd import _lib
    _lib.timing_enable(True)
    try:
        _lib.timing_reset()
        out = fn()
        return out, _lib.timing_read(name)[1]
    finally:
        _lib.timing_enable(False)


def _slice_vjp(geo, zs, row, g, axis="x", cls=None):
    """(A x, A^H g, expand launches) through autograd on propagate_zx(grad="slice")."""
    f = _field(geo, grad=True)

    def run():
        out = _prop(cls).propagate_zx(f, list(zs), row=row, axis=axis, grad="slice", **_grid(geo))
        gx, = torch.autograd.grad(out, f.data, grad_outputs=g)
        return out.detach(), gx

    (out, gx), n = _launches(run)
    return out, gx, n


def _planes_vjp(geo, zs, row, g, axis="x"):
    f = _field(geo, grad=True)
    out = _prop().propagate_zx(f, list(zs), row=row, axis=axis, grad="planes", **_grid(geo))
    gx, = torch.autograd.grad(out, f.data, grad_outputs=g)
    return out.detach(), gx


def _full_adjoint(geo, zs, row, g):
    """The full-plane adjoint: g[k] at row ``row`` of a zero plane through czt_apply(adjoint=True), summed."""
    from quantizationawarethzdoe_amd.propagation import czt_apply
    H, W, out, C, B = geo[:5]
    wl, sp, oh, ow, odx, ody = _cfg(geo)
    res = torch.zeros(B, C, H, W, dtype=torch.complex64, device=_dev())
    G = torch.zeros(B, C, ow, oh, dtype=torch.complex64, device=_dev())
    for k, z in enumerate(zs):
        G[:, :, row, :] = g[k]
        res += czt_apply(G, wl, sp, z, oh, ow, odx, ody, adjoint=True, field_hw=(H, W))
    return res


@pytest.mark.parametrize("geo", GEOMETRIES, **IDS)
def test_adjoint_identity_against_the_native_forward(geo):
    x = _input(geo).to(_dev())
    for row in _rows(geo[2]):
        g = _cotangent(geo, len(ZS), row).to(_dev())
        Ax, AHg, n = _slice_vjp(geo, ZS, row, g)
        assert n == 1 and AHg.shape == x.shape
        err = abs(_dot(Ax, g) - _dot(x, AHg))
        bound = IDENTITY_TOL * float(Ax.norm()) * float(g.norm())
        print(f"czt zx grad {geo[:3]} row {row}: |<Ax,g> - <x,A^H g>| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (geo[:3], row, err, bound)


def _check_gradient(geo, zs, rows):
    from quantizationawarethzdoe_amd.propagation import czt_slice_adjoint
    H, W = geo[:2]
    wl, sp, oh, ow, odx, ody = _cfg(geo)
    want = _oracle_grads(geo, tuple(zs), tuple(rows))
    for row in rows:
        g = _cotangent(geo, len(zs), row).to(_dev())
        got = None
        for k in range(0, len(zs), 256):
            part = czt_slice_adjoint(g[k:k + 256], wl, sp, list(zs[k:k + 256]), row, oh, ow, odx, ody, (H, W))
            got = part if got is None else got + part
        e_or, e_pl = _rel(got, want[row]), _rel(got, _full_adjoint(geo, zs, row, g))
        print(f"czt zx grad {geo[:3]} row {row} Z {len(zs)}: vs oracle {e_or:.3e}, vs full-plane adjoint {e_pl:.3e}")
        assert e_or <= ORACLE_TOL, (geo[:3], row, e_or)
        assert e_pl <= PLANES_TOL, (geo[:3], row, e_pl)


@pytest.mark.parametrize("geo", GEOMETRIES, **IDS)
def test_gradient_vs_oracle_and_full_plane_adjoint(geo):
    _check_gradient(geo, ZS, _rows(geo[2]))


def test_compile_time_2048_point_plan():
    _check_gradient(BIG, ZS[::2], (BIG[2] // 2,))


@pytest.mark.parametrize("geo", GEOMETRIES[:1] + GEOMETRIES[2:3], **IDS)
def test_public_api_slice_vs_planes(geo):
    row = geo[2] // 2
    g = _cotangent(geo, len(ZS), row).to(_dev())
    f = _field(geo, grad=True)
    out, n = _launches(lambda: _prop().propagate_zx(f, list(ZS), row=row, grad="slice", **_grid(geo)))
    assert out.grad_fn is not None and n == 0   # the forward alone launches no expand kernel
    gs, n = _launches(lambda: torch.autograd.grad(out, f.data, grad_outputs=g)[0])
    assert n == 1, "one expand launch for the five-plane sweep"
    (want, gp), n = _launches(lambda: _planes_vjp(geo, ZS, row, g))
    assert n == 0, "grad='planes' never runs the slice adjoint"
    errs = ((out.detach() - want).flatten(1).norm(dim=1) / want.flatten(1).norm(dim=1)).tolist()
    print(f"czt zx grad api {geo[:3]}: values {max(errs):.3e}, gradient {_rel(gs, gp):.3e}")
    assert max(errs) <= PLANES_TOL and _rel(gs, gp) <= PLANES_TOL


def test_sweep_longer_than_max_z():
    """THZ_MAX_Z + 3 planes: the backward crosses the library's 16-plane chunks (the read-add-store
    path) with a 3-plane tail, and the Python chunking: 16 + 1 expand launches."""
    from quantizationawarethzdoe_amd import _lib
    geo, Z = GEOMETRIES[3], _lib.THZ_MAX_Z + 3
    zs = tuple(0.03 + 0.06 * (k / (Z - 1)) ** 1.5 for k in range(Z))
    row = geo[2] // 2
    g = _cotangent(geo, Z, row).to(_dev())
    _, gx, n = _slice_vjp(geo, zs, row, g)
    assert n == 17
    want = _oracle_grads(geo, zs, (row,))[row]
    e_or, e_pl = _rel(gx, want), _rel(gx, _full_adjoint(geo, zs, row, g))
    print(f"czt zx grad Z {Z}: vs oracle {e_or:.3e}, vs full-plane adjoint {e_pl:.3e}")
    assert e_or <= ORACLE_TOL and e_pl <= PLANES_TOL


def test_axis_y_runs_natively_when_dx_equals_dy():
    geo = GEOMETRIES[2]   # 130 x 70, dx = dy
    for row in _rows(geo[2]):
        g = _cotangent(geo, len(ZS), row).to(_dev())
        out, gx, n = _slice_vjp(geo, ZS, row, g, axis="y")
        assert n == 1
        want, gp = _planes_vjp(geo, ZS, row, g, axis="y")
        print(f"czt zx grad axis y row {row}: gradient vs planes {_rel(gx, gp):.3e}")
        assert _rel(out, want) <= PLANES_TOL and _rel(gx, gp) <= PLANES_TOL


def test_axis_y_with_dx_ne_dy_takes_the_planes():
    geo = GEOMETRIES[0]   # dx = 0.25 mm, dy = 0.3 mm: Dm comes from dx on both axes
    for row in _rows(geo[2]):
        g = _cotangent(geo, len(ZS), row).to(_dev())
        out, gx, n = _slice_vjp(geo, ZS, row, g, axis="y")
        assert n == 0
        want, gp = _planes_vjp(geo, ZS, row, g, axis="y")
        assert torch.equal(out, want) and torch.equal(gx, gp)


@pytest.mark.parametrize("Z", [5, 19])
def test_out_is_overwritten(Z):
    from quantizationawarethzdoe_amd.propagation import czt_slice_adjoint
    geo = GEOMETRIES[0]
    H, W, out, C, B = geo[:5]
    wl, sp, oh, ow, odx, ody = _cfg(geo)
    zs = [0.03 + 0.003 * k for k in range(Z)]
    g = _cotangent(geo, Z, 11).to(_dev())
    fresh = czt_slice_adjoint(g, wl, sp, zs, 11, oh, ow, odx, ody, (H, W))
    buf = torch.full((B, C, H, W), float("nan"), dtype=torch.complex64, device=_dev())
    res = czt_slice_adjoint(g, wl, sp, zs, 11, oh, ow, odx, ody, (H, W), out=buf)
    assert res is buf and not torch.isnan(torch.view_as_real(buf)).any()
    assert torch.equal(torch.view_as_real(buf), torch.view_as_real(fresh))


def test_two_backward_calls_are_bit_identical():
    for geo in (GEOMETRIES[0], GEOMETRIES[2]):
        g = _cotangent(geo, len(ZS), 11).to(_dev())
        a = _slice_vjp(geo, ZS, 11, g)[1]
        b = _slice_vjp(geo, ZS, 11, g)[1]
        assert torch.equal(torch.view_as_real(a), torch.view_as_real(b))


def test_input_that_does_not_require_grad():
    geo, row = GEOMETRIES[0], 7
    f = _field(geo)
    got, n = _launches(lambda: _prop().propagate_zx(f, list(ZS), row=row, grad="slice", **_grid(geo)),
                       "czt_slice_collapse")
    assert n == 1 and got.grad_fn is None and not got.requires_grad
    assert torch.equal(got, _prop().propagate_zx(f, list(ZS), row=row, **_grid(geo)))


def test_complex128_falls_back_and_is_differentiable():
    geo, rows = GEOMETRIES[3], _rows(GEOMETRIES[3][2])
    want = _oracle_grads(geo, ZS, rows, True)
    for row in rows:
        f = _field(geo, torch.complex128, grad=True)
        g = _cotangent(geo, len(ZS), row, torch.complex128).to(_dev())

        def run():
            out = _prop().propagate_zx(f, list(ZS), row=row, grad="slice", **_grid(geo))
            return out, torch.autograd.grad(out, f.data, grad_outputs=g)[0]

        (out, gx), n = _launches(run)
        assert n == 0 and out.dtype == gx.dtype == torch.complex128
        err = _rel(gx, want[row])
        print(f"czt zx grad complex128 row {row}: vs oracle {err:.3e}")
        assert err <= F64_TOL


def test_gradient_reaches_a_phase_parameter():
    geo = GEOMETRIES[0]
    H, W, out, C, B = geo[:5]
    amp = _input(geo).abs().to(_dev())
    phi0 = torch.rand(1, 1, H, W, generator=torch.Generator().manual_seed(3)).to(_dev()) * 6.0
    grads = {}
    for mode in ("slice", "planes"):
        phi = phi0.clone().requires_grad_(True)
        f = _field(geo, data=amp * torch.exp(1j * phi))

        def run():
            zx = _prop().propagate_zx(f, list(ZS), grad=mode, **_grid(geo))
            return torch.autograd.grad(zx.abs().square().sum(), phi)[0]

        grads[mode], n = _launches(run)
        assert n == (1 if mode == "slice" else 0)
    err = _rel(grads["slice"], grads["planes"])
    print(f"czt zx grad d phi: slice vs planes {err:.3e}")
    assert grads["slice"].shape == (1, 1, H, W) and err <= PLANES_TOL


def test_vczt_prop_inherits_the_keyword():
    from quantizationawarethzdoe_amd.Props.CZT_Prop import VCZT_prop
    geo = GEOMETRIES[0]
    g = _cotangent(geo, len(ZS), 3).to(_dev())
    a, ga, na = _slice_vjp(geo, ZS, 3, g)
    b, gb, nb = _slice_vjp(geo, ZS, 3, g, cls=VCZT_prop)
    assert na == nb == 1 and torch.equal(a, b) and torch.equal(ga, gb)
