"""CZT z-x slice on the GPU: CZT_prop.propagate_zx (thz_czt_slice_forward: collapse kernel + one
Bluestein line per (z, b, c)) against the fp64 oracle's planes and against the existing HIP planes.

Bound 1: relative L2 per (z, row) against oracle.thz_oracle.czt_forward in fp64, sliced: <= 1e-3,
the project's CZT bound (tests/test_czt_gpu.py).  Bound 2: against propagate_planes(...)[..., row, :]
on the same device: <= 2e-3, the triangle inequality of two results each within 1e-3 of the oracle.
Inputs are seeded complex white noise (every output row carries 0.58 - 1.3 of the mean row energy on
the oracle, so a per-row relative L2 is meaningful).  The oracle sees the fp32-rounded wavelengths,
spacings and distances the kernels are given.
"""
import functools

import pytest
import torch

from oracle import thz_oracle as orc

pytestmark = pytest.mark.gpu

# (H, W, out, C, B, (dx, dy), (odx, ody)): lines that are no multiple of 64, H != W and dx != dy,
# B and C above 1, M >= m (48 -> 64), the runtime FFT plans (np2 = 256, 128, 128, 64)
GEOMETRIES = [
    (72, 100, 40, 2, 2, (0.25e-3, 0.3e-3), (0.1e-3, 0.12e-3)),
    (48, 48, 64, 1, 1, (0.25e-3, 0.25e-3), (0.05e-3, 0.05e-3)),
    (130, 70, 33, 3, 1, (0.25e-3, 0.25e-3), (0.1e-3, 0.1e-3)),
    (20, 24, 20, 1, 2, (0.5e-3, 0.5e-3), (0.2e-3, 0.2e-3)),
]
BIG = (1024, 1024, 256, 1, 1, (0.25e-3, 0.25e-3), (0.25e-3, 0.25e-3))   # np2 = 2048: the compile-time plan
ZS = (0.030, 0.041, 0.055, 0.0725, 0.090)   # 30 ... 90 mm, not uniformly spaced
ORACLE_TOL, PLANES_TOL = 1e-3, 2e-3


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


def _field(geo, dtype=torch.complex64, grad=False):
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    C, spacing = geo[3], geo[5]
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


@functools.lru_cache(maxsize=None)
def _oracle_planes(geo, zs, exact=False):
    """fp64 oracle planes [Z, B, C, outW, outH] (computed once per geometry and sweep, never modified);
    the values the kernels are given: fp32 roundings, or with ``exact`` (the complex128 test) the
    doubles themselves except the input spacing, which ElectricField stores as float32."""
    H, W, out, C, B, spacing, (odx, ody) = geo
    spacing = (_f32(spacing[0]), _f32(spacing[1]))
    r = (lambda v: v) if exact else _f32
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        x = _input(geo, torch.complex128 if exact else torch.complex64).to(torch.complex128)
        lam = torch.tensor([r(v) for v in _lam(C)])
        return torch.stack([orc.czt_forward(x, lam, [r(spacing[0]), r(spacing[1])], r(z), out, out, r(odx), r(ody))
                            for z in zs])
    finally:
        torch.set_default_dtype(old)


@functools.lru_cache(maxsize=None)
def _hip_planes(geo, zs):
    with torch.no_grad():
        return _prop().propagate_planes(_field(geo), list(zs), **_grid(geo)).cpu()


def _rel_per_z(got, want):
    """relative L2 per plane of [Z, B, C, n] slices"""
    got, want = got.to(torch.complex128), want.to(torch.complex128)
    return ((got - want).flatten(1).norm(dim=1) / want.flatten(1).norm(dim=1)).tolist()


def _check(geo, zs, row, got, axis="x"):
    sl = (lambda p: p[..., row, :]) if axis == "x" else (lambda p: p[..., :, row])
    e_or = max(_rel_per_z(got, sl(_oracle_planes(geo, zs))))
    e_pl = max(_rel_per_z(got, sl(_hip_planes(geo, zs))))
    print(f"czt zx {geo[:3]} axis {axis} row {row} Z {len(zs)}: vs oracle {e_or:.3e}, vs planes {e_pl:.3e}")
    assert e_or <= ORACLE_TOL, (geo[:3], row, e_or)
    assert e_pl <= PLANES_TOL, (geo[:3], row, e_pl)


def _native_launches(fn):
    """(result, launches of the collapse kernel) of fn(): whether the slice kernels served the call."""
    from quantizationawarethzdoe_amd import _lib
    _lib.timing_enable(True)
    try:
        _lib.timing_reset()
        out = fn()
        return out, _lib.timing_read("czt_slice_collapse")[1]
    finally:
        _lib.timing_enable(False)


@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: f"{g[0]}x{g[1]}to{g[2]}")
def test_slice_vs_oracle_and_planes(geo):
    prop, field, out = _prop(), _field(geo), geo[2]
    for row in _rows(out):
        got, n = _native_launches(lambda: prop.propagate_zx(field, list(ZS), row=row, **_grid(geo)))
        assert n == 1, "the slice kernels serve a complex64 device field"
        assert got.shape == (len(ZS), geo[4], geo[3], out) and got.dtype == torch.complex64
        _check(geo, ZS, row, got.cpu())
    centre = prop.propagate_zx(field, list(ZS), **_grid(geo))
    assert torch.equal(centre, prop.propagate_zx(field, list(ZS), row=out // 2, **_grid(geo)))


def test_slice_of_a_one_point_output():
    """outH = outW = 1: the output grid is a one-point linspace, its start, so both zoom ranges are
    f2 = f1 (csrc/thz_czt.hip czt_slice_layout, as czt_layout); the only row, against the oracle and
    the planes.  (With f2 = -f1 the chirp rate is off by 2 pi odx dx / (lambda z) and the result by O(1).)"""
    geo = (37, 53, 1, 2, 2, (0.25e-3, 0.3e-3), (0.1e-3, 0.12e-3))
    prop, field = _prop(), _field(geo)
    got, n = _native_launches(lambda: prop.propagate_zx(field, list(ZS), row=0, **_grid(geo)))
    assert n == 1 and got.shape == (len(ZS), 2, 2, 1)
    _check(geo, ZS, 0, got.cpu())


def test_compile_time_2048_point_plan():
    zs = ZS[::2]
    prop, field = _prop(), _field(BIG)
    for row in _rows(BIG[2]):
        _check(BIG, zs, row, prop.propagate_zx(field, list(zs), row=row, **_grid(BIG)).cpu())


def test_sweep_longer_than_max_z():
    """THZ_MAX_Z + 3 planes: crosses the library's 16-plane chunks (with a 3-plane tail in the
    second call) and the Python chunking."""
    from quantizationawarethzdoe_amd import _lib
    geo, Z = GEOMETRIES[3], _lib.THZ_MAX_Z + 3
    zs = tuple(0.03 + 0.06 * (k / (Z - 1)) ** 1.5 for k in range(Z))
    prop, field = _prop(), _field(geo)
    for row in _rows(geo[2]):
        got, n = _native_launches(lambda: prop.propagate_zx(field, list(zs), row=row, **_grid(geo)))
        assert n == 17 and got.shape[0] == Z
        _check(geo, zs, row, got.cpu())


def test_axis_y_runs_natively_when_dx_equals_dy():
    geo = GEOMETRIES[2]   # 130 x 70, dx = dy
    prop, field = _prop(), _field(geo)
    for row in _rows(geo[2]):
        got, n = _native_launches(lambda: prop.propagate_zx(field, list(ZS), row=row, axis="y", **_grid(geo)))
        assert n == 1
        _check(geo, ZS, row, got.cpu(), axis="y")


def test_axis_y_with_dx_ne_dy_slices_the_planes():
    geo = GEOMETRIES[0]   # dx = 0.25 mm, dy = 0.3 mm: Dm comes from dx on both axes
    prop, field = _prop(), _field(geo)
    for row in _rows(geo[2]):
        got, n = _native_launches(lambda: prop.propagate_zx(field, list(ZS), row=row, axis="y", **_grid(geo)))
        assert n == 0
        assert torch.equal(got.cpu(), _hip_planes(geo, ZS)[..., :, row])


def test_input_that_requires_grad_is_differentiable():
    geo, row = GEOMETRIES[0], 7
    prop = _prop()
    f1, f2 = _field(geo, grad=True), _field(geo, grad=True)
    got = prop.propagate_zx(f1, list(ZS), row=row, **_grid(geo))
    assert got.grad_fn is not None
    want = prop.propagate_planes(f2, list(ZS), **_grid(geo))[..., row, :]
    assert torch.equal(got, want)
    g = torch.randn(got.shape, dtype=torch.complex64, generator=torch.Generator().manual_seed(5)).to(_dev())
    g1, = torch.autograd.grad(got, f1.data, grad_outputs=g)
    g2, = torch.autograd.grad(want, f2.data, grad_outputs=g)
    assert float((g1 - g2).norm() / g2.norm()) <= 1e-6
    with torch.no_grad():   # under no_grad the same field takes the slice kernels
        _, n = _native_launches(lambda: prop.propagate_zx(f1, list(ZS), row=row, **_grid(geo)))
    assert n == 1


def test_complex128_field_takes_the_fp64_planes():
    geo = GEOMETRIES[3]
    field = _field(geo, torch.complex128)
    for row in _rows(geo[2]):
        got, n = _native_launches(lambda: _prop().propagate_zx(field, list(ZS), row=row, **_grid(geo)))
        assert n == 0 and got.dtype == torch.complex128
        err = max(_rel_per_z(got.cpu(), _oracle_planes(geo, ZS, True)[..., row, :]))
        print(f"czt zx complex128 row {row}: vs oracle {err:.3e}")
        assert err <= 1e-8   # the project's fp64 CZT bound (tests/test_f64_gpu.py)


def test_vczt_prop_inherits_the_slice():
    from quantizationawarethzdoe_amd.Props.CZT_Prop import VCZT_prop
    geo = GEOMETRIES[0]
    a = _prop().propagate_zx(_field(geo), list(ZS), row=3, **_grid(geo))
    b = _prop(VCZT_prop).propagate_zx(_field(geo), list(ZS), row=3, **_grid(geo))
    assert torch.equal(a, b)
    _check(geo, ZS, 3, b.cpu())


def test_two_native_calls_are_bit_identical():
    """H is split over workgroups in these geometries (4 partial sums of 72 rows, 8 of 130): the
    partial sums are added in a fixed order."""
    for geo in (GEOMETRIES[0], GEOMETRIES[2]):
        prop, field = _prop(), _field(geo)
        a = prop.propagate_zx(field, list(ZS), row=11, **_grid(geo))
        b = prop.propagate_zx(field, list(ZS), row=11, **_grid(geo))
        assert torch.equal(torch.view_as_real(a), torch.view_as_real(b))


def test_propagate_planes_is_forward_per_plane():
    geo = GEOMETRIES[0]
    prop, field = _prop(), _field(geo)
    z0 = prop.z.clone()
    planes = prop.propagate_planes(field, list(ZS), **_grid(geo))
    assert torch.equal(prop.z, z0) and prop._zh == 0.05
    assert planes.shape == (len(ZS), geo[4], geo[3], geo[2], geo[2])
    other = _prop()
    for k, z in enumerate(ZS):
        other.z = z
        assert torch.equal(planes[k], other(field, **_grid(geo)).data)
