"""The native backward of the RSC / VRS z-x slice on the GPU: RSC_prop.propagate_zx(..., grad="slice")
runs the slice kernels forward (rsc_slice_rows / rsc_slice_acc / rsc_slice_line) and their adjoint
backward (thz_rsc_slice_adjoint: rsc_slice_line_adj on the cotangent lines, rsc_slice_acc_adj summing
the planes in the spectrum, rsc_slice_rows_adj), so a loss on the axial map never forms a plane.

Geometries, sweep, ``_lam`` and ``_f32`` are those of tests/test_rsc_zx_gpu.py; inputs and cotangents are
seeded white complex noise.

Bounds (all the project's own):
* adjoint identity against the native forward: |<A x, g> - <x, A^H g>| <= 1e-5 ||A x|| ||g||, the dot
  products in complex128 (tests/test_properties_gpu.py, tests/test_asm_zx_grad_gpu.py);
* against autograd through the fp64 oracle on the fp32-rounded parameters: rel-L2 <= 5e-4, the RSC
  bound of tests/test_rsc_gpu.py.  Pw = 16384 (the 4 x 8192 field) is checked against the full-plane
  adjoint only; its distance to the oracle is printed, not asserted (DESIGN.md section 20 records it);
* against the full-plane adjoint (the cotangent at row p of zero planes through
  rsc_apply(adjoint=True) per z, summed; VRS: through _RscFunction) and between the two ``grad``
  forms: <= 1e-3;
* complex128 (the fp64 planes serve it): <= 1e-10.
"""
import functools

import pytest
import torch

from oracle import thz_oracle as orc
from tests.test_rsc_zx_gpu import (BATCHES, GEOMETRIES, PLANS, VRS, VRS_1200, VRS_4096, VRS_PLAN, ZS, _dev, _f32,
                                   _field, _id, _input, _lam, _prop, _rows)

pytestmark = pytest.mark.gpu

ORACLE_TOL, PLANES_TOL, IDENTITY_TOL, F64_TOL = 5e-4, 1e-3, 1e-5, 1e-10
WIDE = (4, 8192, 1, 1, (0.25e-3, 0.25e-3))   # Pw = 16384: the runtime-plan accumulate, compile-time line and rows
SCALAR = GEOMETRIES + [g for g in PLANS if g != WIDE] + BATCHES
assert WIDE in PLANS
ACC_ADJ = "rsc_slice_acc_adj"


@functools.lru_cache(maxsize=None)
def _cotangent(geo, Z, row, vectorial=False, dtype=torch.complex64):
    """Seeded white cotangent [Z, Bo, C, Wo] (never modified)."""
    H, W, C, B = geo[:4]
    g = torch.Generator().manual_seed(7919 * H + 31 * W + row)
    return torch.randn(Z, 3 if vectorial else B, C, 2 * (W // 2), dtype=torch.complex128, generator=g).to(dtype)


def _ez(x, H, W, dx, z):
    """[Ex, Ey] -> [Ex, Ey, Ez] on the unpadded grid, in the dtype of x (tests/test_rsc_zx_gpu.py)."""
    xs = torch.linspace(-H * dx / 2, H * dx / 2, H)
    ys = torch.linspace(-W * dx / 2, W * dx / 2, W)
    X, Y = torch.meshgrid(xs, ys, indexing="ij")
    rr = torch.sqrt(X ** 2 + Y ** 2 + z ** 2)
    return torch.cat([x[0:1], x[1:2], x[0:1] * X / rr + x[1:2] * Y / rr], 0)


@functools.lru_cache(maxsize=None)
def _oracle_grads(geo, zs, rows, vectorial=False, exact=False):
    """{row: A_row^H g_row} [B, C, H, W] complex128 by autograd through the fp64 oracle's planes, one
    oracle forward per z shared by the rows; computed once and never modified.  The oracle sees the
    values the kernels are given: fp32 roundings, or with ``exact`` (complex128) the doubles themselves
    except the spacing, which ElectricField stores as float32."""
    H, W, C, B, spacing = geo
    dx, dy = _f32(spacing[0]), _f32(spacing[1])
    r = (lambda v: v) if exact else _f32
    dt = torch.complex128 if exact else torch.complex64
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        x = _input(geo, dt).to(torch.complex128).requires_grad_(True)
        lam = torch.tensor([r(v) for v in _lam(C)])
        acc = {p: torch.zeros(B, C, H, W, dtype=torch.complex128) for p in rows}
        for k, z in enumerate(zs):
            z = r(z)
            v = _ez(x, H, W, dx, z) if vectorial else x
            planes = torch.cat([orc.rsc_forward(v[b:b + 1], lam, [dx, dy], z) for b in range(v.shape[0])], 0)
            for p in rows:
                g = _cotangent(geo, len(zs), p, vectorial, dt)[k].to(torch.complex128)
                acc[p] += torch.autograd.grad(planes[:, :, p, :], x, grad_outputs=g, retain_graph=True)[0]
        return acc
    finally:
        torch.set_default_dtype(old)


def _rel(got, want):
    got, want = got.to(torch.complex128).cpu(), want.to(torch.complex128).cpu()
    return float((got - want).norm() / want.norm())


def _dot(a, b):
    return complex(torch.vdot(a.reshape(-1).to(torch.complex128).cpu(), b.reshape(-1).to(torch.complex128).cpu()))


def _launches(fn, name=ACC_ADJ):
    """(result, launches of the accumulate-adjoint kernel) of fn(): whether the native backward ran."""
    from quantizationawarethzdoe_amd import _lib
    _lib.timing_enable(True)
    try:
        _lib.timing_reset()
        out = fn()
        return out, _lib.timing_read(name)[1]
    finally:
        _lib.timing_enable(False)


def _slice_vjp(geo, zs, row, g, axis="x", vectorial=False):
    """(A x, A^H g, accumulate-adjoint launches): autograd on propagate_zx(grad="slice"), or for a
    scalar B > 1 (which RSC_prop refuses as the reference does) the two raw launches."""
    from quantizationawarethzdoe_amd import propagation as P
    if vectorial or geo[3] == 1:
        f = _field(geo, grad=True)

        def run():
            out = _prop(vectorial).propagate_zx(f, list(zs), row=row, axis=axis, grad="slice")
            gx, = torch.autograd.grad(out, f.data, grad_outputs=g)
            return out.detach(), gx
    else:
        assert axis == "x"
        x = _input(geo).to(_dev())

        def run():
            return (P.rsc_slice_apply(x, _lam(geo[2]), geo[4], list(zs), row),
                    P.rsc_slice_adjoint(g, _lam(geo[2]), geo[4], list(zs), row, x.shape))
    (out, gx), n = _launches(run)
    return out, gx, n


def _planes_vjp(geo, zs, row, g, axis="x", vectorial=False):
    f = _field(geo, grad=True)
    (out, gx), n = _launches(lambda: _vjp_of(_prop(vectorial).propagate_zx(f, list(zs), row=row, axis=axis,
                                                                         grad="planes"), f.data, g))
    assert n == 0, "grad='planes' never runs the slice adjoint"
    return out, gx


def _vjp_of(out, x, g):
    gx, = torch.autograd.grad(out, x, grad_outputs=g)
    return out.detach(), gx


def _full_adjoint(geo, zs, row, g, vectorial=False):
    """The full-plane adjoint: g[k] at row ``row`` of a zero plane through rsc_apply(adjoint=True) per z
    (VRS: through _RscFunction, which folds the Ez chain), summed."""
    from quantizationawarethzdoe_amd.propagation import rsc_apply
    from quantizationawarethzdoe_amd.Props.RSC_Prop import _RscFunction
    H, W, C, B = geo[:4]
    wl, sp = tuple(_lam(C)), tuple(geo[4])
    res = torch.zeros(B, C, H, W, dtype=torch.complex64, device=_dev())
    G = torch.zeros(g.shape[1], C, 2 * (H // 2), 2 * (W // 2), dtype=torch.complex64, device=_dev())
    x = _input(geo).to(_dev()).requires_grad_(True)
    for k, z in enumerate(zs):
        G[:, :, row, :] = g[k]
        if vectorial:
            res += torch.autograd.grad(_RscFunction.apply(x, wl, sp, float(z), True), x, grad_outputs=G)[0]
        else:
            res += rsc_apply(G, wl, sp, z, adjoint=True, field_hw=(H, W))
    return res


def _check_identity(geo, vectorial=False, axis="x"):
    x = _input(geo).to(_dev())
    n_out = 2 * (geo[0] // 2) if axis == "x" else 2 * (geo[1] // 2)
    for row in _rows(n_out):
        g = _cotangent(geo, len(ZS), row, vectorial).to(_dev())
        Ax, AHg, n = _slice_vjp(geo, ZS, row, g, vectorial=vectorial)
        assert n == 1 and AHg.shape == x.shape and AHg.dtype == torch.complex64
        err = abs(_dot(Ax, g) - _dot(x, AHg))
        bound = IDENTITY_TOL * float(Ax.norm()) * float(g.norm())
        print(f"rsc zx grad {geo[:4]} vec {vectorial} row {row}: |<Ax,g> - <x,A^H g>| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (geo[:4], row, err, bound)


def _check_gradient(geo, zs, vectorial=False, oracle=True):
    rows = _rows(2 * (geo[0] // 2))
    want = _oracle_grads(geo, tuple(zs), tuple(rows), vectorial)
    for row in rows:
        g = _cotangent(geo, len(zs), row, vectorial).to(_dev())
        _, got, n = _slice_vjp(geo, zs, row, g, vectorial=vectorial)
        assert n == 1
        e_or = _rel(got, want[row])
        e_pl = _rel(got, _full_adjoint(geo, zs, row, g, vectorial))
        print(f"rsc zx grad {geo[:4]} vec {vectorial} row {row}: vs oracle {e_or:.3e}"
              f"{'' if oracle else ' (not asserted)'}, vs full-plane adjoint {e_pl:.3e}")
        if oracle:
            assert e_or <= ORACLE_TOL, (geo[:4], row, e_or)
        assert e_pl <= PLANES_TOL, (geo[:4], row, e_pl)


@pytest.mark.parametrize("geo", SCALAR + [WIDE], ids=_id)
def test_adjoint_identity_against_the_native_forward(geo):
    _check_identity(geo)


@pytest.mark.parametrize("geo", SCALAR, ids=_id)
def test_gradient_vs_oracle_and_full_plane_adjoint(geo):
    _check_gradient(geo, ZS)


def test_widest_line_vs_full_plane_adjoint():
    """Pw = 16384: asserted against the full-plane adjoint; the distance to the oracle is printed."""
    _check_gradient(WIDE, ZS, oracle=False)


@pytest.mark.parametrize("geo", [VRS, VRS_PLAN, VRS_1200, VRS_4096], ids=_id)
def test_vrs_gradient(geo):
    """The identity, both bounds, and consistency: with a zero third cotangent plane the Ex / Ey
    gradients are bit-equal to the scalar slice adjoint of the same two lines (B = 2, raw launch)."""
    from quantizationawarethzdoe_amd import propagation as P
    H, W, C = geo[:3]
    _check_identity(geo, vectorial=True)
    _check_gradient(geo, ZS, vectorial=True)
    for row in _rows(2 * (H // 2)):
        g = _cotangent(geo, len(ZS), row, True).to(_dev()).clone()
        g[:, 2] = 0
        vec = P.rsc_slice_adjoint(g, _lam(C), geo[4], list(ZS), row, (2, C, H, W), vectorial=True)
        sca = P.rsc_slice_adjoint(g[:, :2].contiguous(), _lam(C), geo[4], list(ZS), row, (2, C, H, W))
        assert torch.equal(vec, sca), (geo[:4], row)


@pytest.mark.parametrize("geo,vectorial", [(GEOMETRIES[0], False), (GEOMETRIES[3], False), (VRS, True)],
                         ids=["72x100", "20x24", "vrs40x48"])
def test_public_slice_against_planes(geo, vectorial):
    """Values and gradients of the two ``grad`` forms; the forward alone launches no adjoint kernel."""
    for row in _rows(2 * (geo[0] // 2)):
        g = _cotangent(geo, len(ZS), row, vectorial).to(_dev())
        f = _field(geo, grad=True)
        out, n = _launches(lambda: _prop(vectorial).propagate_zx(f, list(ZS), row=row, grad="slice"))
        assert n == 0 and out.grad_fn is not None
        _, fwd = _launches(lambda: _prop(vectorial).propagate_zx(f, list(ZS), row=row, grad="slice"), "rsc_slice_acc")
        assert fwd == 1, "grad='slice' runs the slice kernels forward on a field that requires grad"
        o1, g1, n = _slice_vjp(geo, ZS, row, g, vectorial=vectorial)
        o2, g2 = _planes_vjp(geo, ZS, row, g, vectorial=vectorial)
        assert n == 1
        ev, eg = _rel(o1, o2), _rel(g1, g2)
        print(f"rsc zx grad {geo[:4]} vec {vectorial} row {row}: slice vs planes values {ev:.3e}, gradients {eg:.3e}")
        assert ev <= PLANES_TOL and eg <= PLANES_TOL, (row, ev, eg)


def test_sweep_longer_than_max_z():
    """THZ_MAX_Z + 3 planes on 20 x 24: the Python chunking gives calls of 256 and 3 planes, the library
    cuts the first into eight 32-plane chunks (the read-add-store of S): nine accumulate-adjoint launches."""
    from quantizationawarethzdoe_amd import _lib
    geo, Z = GEOMETRIES[3], _lib.THZ_MAX_Z + 3
    zs = tuple(0.03 + 0.06 * (k / (Z - 1)) ** 1.5 for k in range(Z))
    rows = _rows(geo[0])
    want = _oracle_grads(geo, zs, tuple(rows))
    for row in rows:
        g = _cotangent(geo, Z, row).to(_dev())
        out, got, n = _slice_vjp(geo, zs, row, g)
        assert n == 9 and out.shape[0] == Z
        err = _rel(got, want[row])
        print(f"rsc zx grad Z {Z} row {row}: vs oracle {err:.3e}")
        assert err <= ORACLE_TOL


@pytest.mark.parametrize("vectorial", [False, True], ids=["rsc", "vrs"])
def test_axis_y_against_planes(vectorial):
    geo = VRS if vectorial else GEOMETRIES[0]   # dx != dy: the kernel's grid takes dx on both axes
    H, W, C = geo[:3]
    for row in _rows(2 * (W // 2)):
        gen = torch.Generator().manual_seed(17 + row)
        g = torch.randn(len(ZS), 3 if vectorial else 1, C, 2 * (H // 2), dtype=torch.complex64, generator=gen).to(_dev())
        o1, g1, n = _slice_vjp(geo, ZS, row, g, axis="y", vectorial=vectorial)
        o2, g2 = _planes_vjp(geo, ZS, row, g, axis="y", vectorial=vectorial)
        assert n == 1 and o1.shape == o2.shape == g.shape
        ev, eg = _rel(o1, o2), _rel(g1, g2)
        print(f"rsc zx grad axis y vec {vectorial} row {row}: values {ev:.3e}, gradients {eg:.3e}")
        assert ev <= PLANES_TOL and eg <= PLANES_TOL, (row, ev, eg)


@pytest.mark.parametrize("Z", [5, 37])
def test_out_buffer_is_overwritten(Z):
    """grad_in may be uninitialised memory: a NaN-filled ``out`` is overwritten, bit-equal to a fresh
    call, with one chunk (Z = 5) and with the read-add-store chunks (Z = 37); scalar and VRS."""
    from quantizationawarethzdoe_amd import propagation as P
    zs = [0.03 + 0.06 * k / Z for k in range(Z)]
    for geo, vec in ((GEOMETRIES[0], False), (VRS, True)):
        H, W, C, B = geo[:4]
        g = _cotangent(geo, Z, 3, vec).to(_dev())
        fresh = P.rsc_slice_adjoint(g, _lam(C), geo[4], zs, 3, (B, C, H, W), vec)
        buf = torch.full((B, C, H, W), float("nan"), dtype=torch.complex64, device=_dev())
        got = P.rsc_slice_adjoint(g, _lam(C), geo[4], zs, 3, (B, C, H, W), vec, out=buf)
        assert got is buf and torch.isfinite(torch.view_as_real(buf)).all()
        assert torch.equal(torch.view_as_real(buf), torch.view_as_real(fresh))
        with pytest.raises(ValueError, match="out must be"):
            P.rsc_slice_adjoint(g, _lam(C), geo[4], zs, 3, (B, C, H, W), vec, out=buf[..., :-1])
        with pytest.raises(ValueError, match="gradient"):
            P.rsc_slice_adjoint(g[:-1], _lam(C), geo[4], zs, 3, (B, C, H, W), vec)


def test_two_backward_calls_are_bit_identical():
    for geo, vec in ((GEOMETRIES[0], False), (GEOMETRIES[2], False), (PLANS[0], False), (VRS, True),
                     (VRS_PLAN, True)):
        g = _cotangent(geo, len(ZS), 1, vec).to(_dev())
        a, b = _slice_vjp(geo, ZS, 1, g, vectorial=vec)[1], _slice_vjp(geo, ZS, 1, g, vectorial=vec)[1]
        assert torch.equal(torch.view_as_real(a), torch.view_as_real(b)), geo[:4]


def test_field_without_grad_takes_the_slice_kernels():
    geo, row = GEOMETRIES[0], 7
    f = _field(geo)
    got, n = _launches(lambda: _prop().propagate_zx(f, list(ZS), row=row, grad="slice"), "rsc_slice_acc")
    assert n == 1 and got.grad_fn is None and not got.requires_grad
    assert torch.equal(torch.view_as_real(got), torch.view_as_real(_prop().propagate_zx(f, list(ZS), row=row)))


def test_complex128_takes_the_fp64_planes():
    geo = GEOMETRIES[3]
    rows = _rows(geo[0])
    want = _oracle_grads(geo, ZS, tuple(rows), False, True)
    for row in rows:
        f = _field(geo, torch.complex128, grad=True)
        g = _cotangent(geo, len(ZS), row, False, torch.complex128).to(_dev())
        (out, gx), n = _launches(lambda: _vjp_of(_prop().propagate_zx(f, list(ZS), row=row, grad="slice"), f.data, g))
        assert n == 0 and out.dtype == gx.dtype == torch.complex128
        err = _rel(gx, want[row])
        print(f"rsc zx grad complex128 row {row}: vs oracle {err:.3e}")
        assert err <= F64_TOL


def test_gradient_reaches_a_phase_parameter():
    """field = amp exp(i phi), loss = sum |zx|^2: d loss / d phi through grad="slice" against "planes"."""
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    geo = GEOMETRIES[0]
    H, W, C = geo[:3]
    amp = _input(geo).abs().to(_dev())
    phi0 = _input(geo).angle().to(_dev())
    grads = {}
    for form in ("slice", "planes"):
        phi = phi0.clone().requires_grad_(True)
        data = (amp * torch.exp(1j * phi)).to(torch.complex64)
        f = ElectricField(data, wavelengths=_lam(C), spacing=list(geo[4]), device=_dev())
        loss, n = _launches(lambda: _backward_of(_prop().propagate_zx(f, list(ZS), row=H // 2, grad=form)))
        assert n == (1 if form == "slice" else 0)
        grads[form] = phi.grad.detach().clone()
    err = float((grads["slice"] - grads["planes"]).norm() / grads["planes"].norm())
    print(f"rsc zx grad phase parameter: slice vs planes {err:.3e}")
    assert grads["slice"].dtype == torch.float32 and err <= PLANES_TOL


def _backward_of(zx):
    loss = zx.abs().square().sum()
    loss.backward()
    return loss.detach()
