"""RSC / VRS z-x slice on the GPU: RSC_prop.propagate_zx (thz_rsc_slice_forward: the input rows'
spectra once, per plane H kernel rows transformed and accumulated, one inverse line per (z, b, c))
against the fp64 oracle's planes and against the existing HIP planes.

Bound 1: relative L2 per (z, row) against oracle.thz_oracle.rsc_forward in fp64, sliced: <= 5e-4, the
project's RSC bound (tests/test_rsc_gpu.py).  Bound 2: against
propagate_planes(...)[..., row, :] on the same device: <= 1e-3, the triangle inequality of two results
each within Bound 1.  Inputs are seeded complex white noise (every output row carries 0.40 - 1.8 of the
mean row energy on the oracle, so a per-row relative L2 is meaningful).  The oracle sees the
fp32-rounded wavelengths, spacings and distances the kernels are given.
"""
import functools

import pytest
import torch

from oracle import thz_oracle as orc

pytestmark = pytest.mark.gpu

# (H, W, C, B, (dx, dy)): H != W and dx != dy, C and B above 1, odd sizes (Pw = 93, Ph = 65), lines
# that are no multiple of 64 -- all on the runtime FFT plan (Pw = 200, 93, 140, 48)
GEOMETRIES = [
    (72, 100, 2, 1, (0.25e-3, 0.3e-3)),
    (33, 47, 1, 2, (0.25e-3, 0.25e-3)),
    (130, 70, 3, 1, (0.25e-3, 0.25e-3)),
    (20, 24, 1, 1, (0.5e-3, 0.5e-3)),
]
# the compile-time plans Pw = 1024, 2048, 4096 and 8192 (last-stage radices 4, 8, 16, 2; no transform
# runs along H: H stays tiny), and Pw = 16384, whose accumulate kernel runs the runtime plan next to
# compile-time row and line kernels
PLANS = [
    (24, 512, 1, 1, (0.25e-3, 0.25e-3)),
    (16, 1024, 1, 1, (0.25e-3, 0.25e-3)),
    (4, 8192, 1, 1, (0.25e-3, 0.25e-3)),
    (4, 2048, 1, 1, (0.25e-3, 0.25e-3)),
    (4, 4096, 1, 1, (0.25e-3, 0.25e-3)),
]
# more than one output plane per call (through rsc_slice_apply): a runtime-plan width inside
# [1024, 8192] (Pw = 1200: one plane per accumulate workgroup), and the compile-time tiles of two
# (B = 2; B = 4: two tiles of two) and three planes (B = 5: tiles of three and two, one slot idle)
BATCHES = [
    (8, 600, 1, 2, (0.25e-3, 0.25e-3)),
    (8, 512, 1, 2, (0.25e-3, 0.25e-3)),
    (6, 512, 1, 4, (0.25e-3, 0.25e-3)),
    (6, 512, 1, 5, (0.25e-3, 0.25e-3)),
]
VRS = (40, 48, 2, 2, (0.25e-3, 0.3e-3))      # Ex, Ey planes in, three planes out; Pw = 96
VRS_PLAN = (12, 512, 1, 2, (0.25e-3, 0.25e-3))   # Pw = 1024: three planes per accumulate workgroup
VRS_1200 = (8, 600, 2, 2, (0.25e-3, 0.25e-3))    # Pw = 1200: the runtime plan inside [1024, 8192]
VRS_4096 = (4, 2048, 1, 2, (0.25e-3, 0.25e-3))   # Pw = 4096: the radix-16 last stage, three planes
ZS = (0.030, 0.041, 0.055, 0.0725, 0.090)   # 30 ... 90 mm, not uniformly spaced
ORACLE_TOL, PLANES_TOL = 5e-4, 1e-3


def _dev():
    return torch.device("cuda:0")


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def _lam(C):
    return [1e-3 * (1 + 0.1 * c) for c in range(C)]


def _rows(n):
    return (0, n // 2, n - 1)


def _id(g):
    return f"{g[0]}x{g[1]}" + (f"xB{g[3]}" if g[3] > 2 else "")


@functools.lru_cache(maxsize=None)
def _input(geo, dtype=torch.complex64):
    H, W, C, B = geo[:4]
    g = torch.Generator().manual_seed(1000 * H + W)
    return torch.randn(B, C, H, W, dtype=torch.complex128, generator=g).to(dtype)


def _field(geo, dtype=torch.complex64, grad=False, data=None):
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    C, spacing = geo[2], geo[4]
    data = (_input(geo, dtype) if data is None else data).to(_dev())
    if grad:
        data.requires_grad_(True)
    wl = _lam(C)
    if dtype == torch.complex128:
        wl = torch.tensor(wl, dtype=torch.float64)
    elif C == 1:
        wl = wl[0]
    return ElectricField(data, wavelengths=wl, spacing=list(spacing), device=_dev())


def _prop(vectorial=False):
    from quantizationawarethzdoe_amd.Props.RSC_Prop import RSC_prop, VRS_prop
    return (VRS_prop if vectorial else RSC_prop)(z_distance=0.05, device=_dev())


@functools.lru_cache(maxsize=None)
def _oracle_planes(geo, zs, vectorial=False, exact=False):
    """fp64 oracle planes [Z, Bo, C, Ho, Wo] (computed once per geometry and sweep, never modified) at
    the values the kernels are given: fp32 roundings, or with ``exact`` (the complex128 test) the
    doubles themselves except the spacing, which ElectricField stores as float32.  VRS: Ez = Ex x / r +
    Ey y / r on the unpadded grid, then the scalar convolution per component
    (test_vrs_matches_oracle_componentwise)."""
    H, W, C, B, spacing = geo
    dx, dy = _f32(spacing[0]), _f32(spacing[1])
    r = (lambda v: v) if exact else _f32
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        x = _input(geo, torch.complex128 if exact else torch.complex64).to(torch.complex128)
        lam = torch.tensor([r(v) for v in _lam(C)])
        planes = []
        for z in zs:
            z = r(z)
            v = x
            if vectorial:
                xs = torch.linspace(-H * dx / 2, H * dx / 2, H)
                ys = torch.linspace(-W * dx / 2, W * dx / 2, W)
                X, Y = torch.meshgrid(xs, ys, indexing="ij")
                rr = torch.sqrt(X ** 2 + Y ** 2 + z ** 2)
                v = torch.cat([x[0:1], x[1:2], x[0:1] * X / rr + x[1:2] * Y / rr], 0)
            planes.append(torch.cat([orc.rsc_forward(v[b:b + 1], lam, [dx, dy], z) for b in range(v.shape[0])], 0))
        return torch.stack(planes)
    finally:
        torch.set_default_dtype(old)


@functools.lru_cache(maxsize=None)
def _hip_planes(geo, zs, vectorial=False):
    """The existing HIP planes [Z, Bo, C, Ho, Wo]: propagate_planes, or for a scalar B > 1 (which
    RSC_prop refuses as the reference does) the raw plane launch per z."""
    from quantizationawarethzdoe_amd import propagation as P
    with torch.no_grad():
        if vectorial or geo[3] == 1:
            return _prop(vectorial).propagate_planes(_field(geo), list(zs)).cpu()
        x = _input(geo).to(_dev())
        return torch.stack([P.rsc_apply(x, _lam(geo[2]), geo[4], z) for z in zs]).cpu()


def _zx(geo, zs, row=None, axis="x", vectorial=False):
    """The slice through the public method, or for a scalar B > 1 through the raw launch."""
    from quantizationawarethzdoe_amd import propagation as P
    if vectorial or geo[3] == 1:
        return _prop(vectorial).propagate_zx(_field(geo), list(zs), row=row, axis=axis)
    assert axis == "x"
    return P.rsc_slice_apply(_input(geo).to(_dev()), _lam(geo[2]), geo[4], list(zs), row)


def _rel_per_z(got, want):
    """relative L2 per plane of [Z, B, C, n] slices"""
    got, want = got.to(torch.complex128), want.to(torch.complex128)
    return ((got - want).flatten(1).norm(dim=1) / want.flatten(1).norm(dim=1)).tolist()


def _check(geo, zs, row, got, axis="x", vectorial=False):
    sl = (lambda p: p[..., row, :]) if axis == "x" else (lambda p: p[..., :, row])
    e_or = max(_rel_per_z(got, sl(_oracle_planes(geo, zs, vectorial))))
    e_pl = max(_rel_per_z(got, sl(_hip_planes(geo, zs, vectorial))))
    print(f"rsc zx {geo[:4]} vec {vectorial} axis {axis} row {row} Z {len(zs)}: vs oracle {e_or:.3e}, "
          f"vs planes {e_pl:.3e}")
    assert e_or <= ORACLE_TOL, (geo[:4], row, e_or)
    assert e_pl <= PLANES_TOL, (geo[:4], row, e_pl)


def _native_launches(fn):
    """(result, launches of the accumulate kernel) of fn(): whether the slice kernels served the call."""
    from quantizationawarethzdoe_amd import _lib
    _lib.timing_enable(True)
    try:
        _lib.timing_reset()
        out = fn()
        return out, _lib.timing_read("rsc_slice_acc")[1]
    finally:
        _lib.timing_enable(False)


@pytest.mark.parametrize("geo", GEOMETRIES + PLANS + BATCHES, ids=_id)
def test_slice_vs_oracle_and_planes(geo):
    H, W, C, B = geo[:4]
    Ho, Wo = 2 * (H // 2), 2 * (W // 2)
    for row in _rows(Ho):
        got, n = _native_launches(lambda: _zx(geo, ZS, row))
        assert n == 1, "the slice kernels serve a complex64 device field"
        assert got.shape == (len(ZS), B, C, Wo) and got.dtype == torch.complex64
        _check(geo, ZS, row, got.cpu())
    if B == 1:
        assert torch.equal(_zx(geo, ZS), _zx(geo, ZS, Ho // 2))


@pytest.mark.parametrize("geo", [VRS, VRS_PLAN, VRS_1200, VRS_4096], ids=_id)
def test_vrs_three_planes(geo):
    """All three planes within both bounds (Ez carries each plane's own z in its r), and planes 0 / 1
    bit-equal to RSC_prop's slice of a B = 1 field holding Ex, resp. Ey."""
    H, W, C = geo[:3]
    for row in _rows(2 * (H // 2)):
        got, n = _native_launches(lambda: _zx(geo, ZS, row, vectorial=True))
        assert n == 1 and got.shape == (len(ZS), 3, C, 2 * (W // 2))
        _check(geo, ZS, row, got.cpu(), vectorial=True)
        for b in (0, 1):
            one = _prop().propagate_zx(_field(geo, data=_input(geo)[b:b + 1]), list(ZS), row=row)
            assert torch.equal(torch.view_as_real(got[:, b:b + 1]), torch.view_as_real(one)), (row, b)


def test_axis_y_runs_natively_scalar():
    geo = GEOMETRIES[0]   # H != W, dx != dy: the kernel's grid takes dx on both axes
    for row in _rows(2 * (geo[1] // 2)):
        got, n = _native_launches(lambda: _zx(geo, ZS, row, axis="y"))
        assert n == 1 and got.shape == (len(ZS), 1, geo[2], 2 * (geo[0] // 2))
        _check(geo, ZS, row, got.cpu(), axis="y")
    assert torch.equal(_zx(geo, ZS, axis="y"), _zx(geo, ZS, (2 * (geo[1] // 2)) // 2, axis="y"))


def test_axis_y_runs_natively_vrs():
    geo = VRS
    for row in _rows(2 * (geo[1] // 2)):
        got, n = _native_launches(lambda: _zx(geo, ZS, row, axis="y", vectorial=True))
        assert n == 1 and got.shape == (len(ZS), 3, geo[2], 2 * (geo[0] // 2))
        _check(geo, ZS, row, got.cpu(), axis="y", vectorial=True)


def test_sweep_longer_than_max_z():
    """THZ_MAX_Z + 3 planes: crosses the library's 32-plane chunks (8 in the first call, a 3-plane
    one in the second) and the Python chunking."""
    from quantizationawarethzdoe_amd import _lib
    geo, Z = GEOMETRIES[3], _lib.THZ_MAX_Z + 3
    zs = tuple(0.03 + 0.06 * (k / (Z - 1)) ** 1.5 for k in range(Z))
    for row in _rows(geo[0]):
        got, n = _native_launches(lambda: _zx(geo, zs, row))
        assert n == 9 and got.shape[0] == Z
        _check(geo, zs, row, got.cpu())


def test_two_native_calls_are_bit_identical():
    """The input rows are split over workgroups in these geometries (hs = 32 of 72 rows, 21 of 130, 24
    of 24 at Pw = 1024, 4 of 4 at Pw = 16384): the partial sums are added in a fixed order."""
    for geo in (GEOMETRIES[0], GEOMETRIES[2], PLANS[0], PLANS[2]):
        a, b = _zx(geo, ZS, 1), _zx(geo, ZS, 1)
        assert torch.equal(torch.view_as_real(a), torch.view_as_real(b))
    a, b = _zx(VRS_PLAN, ZS, 1, vectorial=True), _zx(VRS_PLAN, ZS, 1, vectorial=True)
    assert torch.equal(torch.view_as_real(a), torch.view_as_real(b))


def test_input_that_requires_grad_is_differentiable():
    geo, row = GEOMETRIES[0], 7
    prop = _prop()
    f1, f2 = _field(geo, grad=True), _field(geo, grad=True)
    got, n = _native_launches(lambda: prop.propagate_zx(f1, list(ZS), row=row))
    assert n == 0 and got.grad_fn is not None
    want = prop.propagate_planes(f2, list(ZS))[..., row, :]
    assert torch.equal(got, want)
    g = torch.randn(got.shape, dtype=torch.complex64, generator=torch.Generator().manual_seed(5)).to(_dev())
    g1, = torch.autograd.grad(got, f1.data, grad_outputs=g)
    g2, = torch.autograd.grad(want, f2.data, grad_outputs=g)
    assert float((g1 - g2).norm() / g2.norm()) <= 1e-6
    with torch.no_grad():   # under no_grad the same field takes the slice kernels
        _, n = _native_launches(lambda: prop.propagate_zx(f1, list(ZS), row=row))
    assert n == 1


def test_complex128_field_takes_the_fp64_planes():
    geo = GEOMETRIES[3]
    field = _field(geo, torch.complex128)
    for row in _rows(geo[0]):
        got, n = _native_launches(lambda: _prop().propagate_zx(field, list(ZS), row=row))
        assert n == 0 and got.dtype == torch.complex128
        err = max(_rel_per_z(got.cpu(), _oracle_planes(geo, ZS, False, True)[..., row, :]))
        print(f"rsc zx complex128 row {row}: vs oracle {err:.3e}")
        assert err <= 1e-10   # the project's fp64 RSC bound


def test_propagate_planes_is_forward_per_plane():
    for geo, vec in ((GEOMETRIES[0], False), (VRS, True)):
        prop, field = _prop(vec), _field(geo)
        z0 = prop.z.clone()
        planes = prop.propagate_planes(field, list(ZS))
        assert torch.equal(prop.z, z0) and prop._zh == 0.05
        assert planes.shape == (len(ZS), 3 if vec else 1, geo[2], 2 * (geo[0] // 2), 2 * (geo[1] // 2))
        other = _prop(vec)
        for k, z in enumerate(ZS):
            other.z = z
            assert torch.equal(planes[k], other(field).data)


def test_empty_window_and_no_output_row():
    """W = 1: the reference's [..., W:] window is empty -> [Z, Bo, C, 0] without a launch.  H = 1: no
    output row to take."""
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    x = torch.ones(1, 2, 8, 1, dtype=torch.complex64, device=_dev())
    field = ElectricField(x, wavelengths=_lam(2), spacing=[1e-3, 1e-3], device=_dev())
    got, n = _native_launches(lambda: _prop().propagate_zx(field, list(ZS)))
    assert n == 0 and got.shape == (len(ZS), 1, 2, 0) and got.dtype == torch.complex64
    x = torch.ones(1, 2, 1, 8, dtype=torch.complex64, device=_dev())
    field = ElectricField(x, wavelengths=_lam(2), spacing=[1e-3, 1e-3], device=_dev())
    with pytest.raises(ValueError, match=r"\[0, 0\)"):
        _prop().propagate_zx(field, list(ZS))
