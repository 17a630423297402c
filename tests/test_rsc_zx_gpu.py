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

from tests import rsc_zx_cases as zc
from tests.gpu_util import dev as _dev

pytestmark = pytest.mark.gpu

ORACLE_TOL, PLANES_TOL = 5e-4, 1e-3




@functools.lru_cache(maxsize=None)
def _hip_planes(geo, zs, vectorial=False):
    """The existing HIP planes [Z, Bo, C, Ho, Wo]: propagate_planes, or for a scalar B > 1 (which
    RSC_prop refuses as the reference does) the raw plane launch per z."""
    from quantizationawarethzdoe_amd import propagation as P
    with torch.no_grad():
        if vectorial or geo[3] == 1:
            return zc.prop(vectorial).propagate_planes(zc.field(geo), list(zs)).cpu()
        x = zc.white_input(geo).to(_dev())
        return torch.stack([P.rsc_apply(x, zc.synthetic_lam(geo[2]), geo[4], z) for z in zs]).cpu()


def _zx(geo, zs, row=None, axis="x", vectorial=False):
    """The slice through the public method, or for a scalar B > 1 through the raw launch."""
    from quantizationawarethzdoe_amd import propagation as P
    if vectorial or geo[3] == 1:
        return zc.prop(vectorial).propagate_zx(zc.field(geo), list(zs), row=row, axis=axis)
    assert axis == "x"
    return P.rsc_slice_apply(zc.white_input(geo).to(_dev()), zc.synthetic_lam(geo[2]), geo[4], list(zs), row)


def _rel_per_z(got, want):
    """relative L2 per plane of [Z, B, C, n] slices"""
    got, want = got.to(torch.complex128), want.to(torch.complex128)
    return ((got - want).flatten(1).norm(dim=1) / want.flatten(1).norm(dim=1)).tolist()


def _check(geo, zs, row, got, axis="x", vectorial=False):
    sl = (lambda p: p[..., row, :]) if axis == "x" else (lambda p: p[..., :, row])
    e_or = max(_rel_per_z(got, sl(zc.oracle_planes(geo, zs, vectorial))))
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


@pytest.mark.parametrize("geo", zc.GEOMETRIES + zc.PLANS + zc.BATCHES, ids=zc.case_id)
def test_slice_vs_oracle_and_planes(geo):
    H, W, C, B = geo[:4]
    Ho, Wo = 2 * (H // 2), 2 * (W // 2)
    for row in zc.rows(Ho):
        got, n = _native_launches(lambda: _zx(geo, zc.ZS, row))
        assert n == 1, "the slice kernels serve a complex64 device field"
        assert got.shape == (len(zc.ZS), B, C, Wo) and got.dtype == torch.complex64
        _check(geo, zc.ZS, row, got.cpu())
    if B == 1:
        assert torch.equal(_zx(geo, zc.ZS), _zx(geo, zc.ZS, Ho // 2))


@pytest.mark.parametrize("geo", [zc.VRS, zc.VRS_PLAN, zc.VRS_1200, zc.VRS_4096], ids=zc.case_id)
def test_vrs_three_planes(geo):
    """All three planes within both bounds (Ez carries each plane's own z in its r), and planes 0 / 1
    bit-equal to RSC_prop's slice of a B = 1 field holding Ex, resp. Ey."""
    H, W, C = geo[:3]
    for row in zc.rows(2 * (H // 2)):
        got, n = _native_launches(lambda: _zx(geo, zc.ZS, row, vectorial=True))
        assert n == 1 and got.shape == (len(zc.ZS), 3, C, 2 * (W // 2))
        _check(geo, zc.ZS, row, got.cpu(), vectorial=True)
        for b in (0, 1):
            one = zc.prop().propagate_zx(zc.field(geo, data=zc.white_input(geo)[b:b + 1]), list(zc.ZS), row=row)
            assert torch.equal(torch.view_as_real(got[:, b:b + 1]), torch.view_as_real(one)), (row, b)


def test_axis_y_runs_natively_scalar():
    geo = zc.GEOMETRIES[0]   # H != W, dx != dy: the kernel's grid takes dx on both axes
    for row in zc.rows(2 * (geo[1] // 2)):
        got, n = _native_launches(lambda: _zx(geo, zc.ZS, row, axis="y"))
        assert n == 1 and got.shape == (len(zc.ZS), 1, geo[2], 2 * (geo[0] // 2))
        _check(geo, zc.ZS, row, got.cpu(), axis="y")
    assert torch.equal(_zx(geo, zc.ZS, axis="y"), _zx(geo, zc.ZS, (2 * (geo[1] // 2)) // 2, axis="y"))


def test_axis_y_runs_natively_vrs():
    geo = zc.VRS
    for row in zc.rows(2 * (geo[1] // 2)):
        got, n = _native_launches(lambda: _zx(geo, zc.ZS, row, axis="y", vectorial=True))
        assert n == 1 and got.shape == (len(zc.ZS), 3, geo[2], 2 * (geo[0] // 2))
        _check(geo, zc.ZS, row, got.cpu(), axis="y", vectorial=True)


def test_sweep_longer_than_max_z():
    """THZ_MAX_Z + 3 planes: crosses the library's 32-plane chunks (8 in the first call, a 3-plane
    one in the second) and the Python chunking."""
    from quantizationawarethzdoe_amd import _lib
    geo, Z = zc.GEOMETRIES[3], _lib.THZ_MAX_Z + 3
    zs = tuple(0.03 + 0.06 * (k / (Z - 1)) ** 1.5 for k in range(Z))
    for row in zc.rows(geo[0]):
        got, n = _native_launches(lambda: _zx(geo, zs, row))
        assert n == 9 and got.shape[0] == Z
        _check(geo, zs, row, got.cpu())


def test_two_native_calls_are_bit_identical():
    """The input rows are split over workgroups in these geometries (hs = 32 of 72 rows, 21 of 130, 24
    of 24 at Pw = 1024, 4 of 4 at Pw = 16384): the partial sums are added in a fixed order."""
    for geo in (zc.GEOMETRIES[0], zc.GEOMETRIES[2], zc.PLANS[0], zc.PLANS[2]):
        a, b = _zx(geo, zc.ZS, 1), _zx(geo, zc.ZS, 1)
        assert torch.equal(torch.view_as_real(a), torch.view_as_real(b))
    a, b = _zx(zc.VRS_PLAN, zc.ZS, 1, vectorial=True), _zx(zc.VRS_PLAN, zc.ZS, 1, vectorial=True)
    assert torch.equal(torch.view_as_real(a), torch.view_as_real(b))


def test_input_that_requires_grad_is_differentiable():
    geo, row = zc.GEOMETRIES[0], 7
    prop = zc.prop()
    f1, f2 = zc.field(geo, grad=True), zc.field(geo, grad=True)
    got, n = _native_launches(lambda: prop.propagate_zx(f1, list(zc.ZS), row=row))
    assert n == 0 and got.grad_fn is not None
    want = prop.propagate_planes(f2, list(zc.ZS))[..., row, :]
    assert torch.equal(got, want)
    g = torch.randn(got.shape, dtype=torch.complex64, generator=torch.Generator().manual_seed(5)).to(_dev())
    g1, = torch.autograd.grad(got, f1.data, grad_outputs=g)
    g2, = torch.autograd.grad(want, f2.data, grad_outputs=g)
    assert float((g1 - g2).norm() / g2.norm()) <= 1e-6
    with torch.no_grad():   # under no_grad the same field takes the slice kernels
        _, n = _native_launches(lambda: prop.propagate_zx(f1, list(zc.ZS), row=row))
    assert n == 1


def test_complex128_field_takes_the_fp64_planes():
    geo = zc.GEOMETRIES[3]
    field = zc.field(geo, torch.complex128)
    for row in zc.rows(geo[0]):
        got, n = _native_launches(lambda: zc.prop().propagate_zx(field, list(zc.ZS), row=row))
        assert n == 0 and got.dtype == torch.complex128
        err = max(_rel_per_z(got.cpu(), zc.oracle_planes(geo, zc.ZS, False, True)[..., row, :]))
        print(f"rsc zx complex128 row {row}: vs oracle {err:.3e}")
        assert err <= 1e-10   # the project's fp64 RSC bound


def test_propagate_planes_is_forward_per_plane():
    for geo, vec in ((zc.GEOMETRIES[0], False), (zc.VRS, True)):
        prop, field = zc.prop(vec), zc.field(geo)
        z0 = prop.z.clone()
        planes = prop.propagate_planes(field, list(zc.ZS))
        assert torch.equal(prop.z, z0) and prop._zh == 0.05
        assert planes.shape == (len(zc.ZS), 3 if vec else 1, geo[2], 2 * (geo[0] // 2), 2 * (geo[1] // 2))
        other = zc.prop(vec)
        for k, z in enumerate(zc.ZS):
            other.z = z
            assert torch.equal(planes[k], other(field).data)


def test_empty_window_and_no_output_row():
    """W = 1: the reference's [..., W:] window is empty -> [Z, Bo, C, 0] without a launch.  H = 1: no
    output row to take."""
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    x = torch.ones(1, 2, 8, 1, dtype=torch.complex64, device=_dev())
    field = ElectricField(x, wavelengths=zc.synthetic_lam(2), spacing=[1e-3, 1e-3], device=_dev())
    got, n = _native_launches(lambda: zc.prop().propagate_zx(field, list(zc.ZS)))
    assert n == 0 and got.shape == (len(zc.ZS), 1, 2, 0) and got.dtype == torch.complex64
    x = torch.ones(1, 2, 1, 8, dtype=torch.complex64, device=_dev())
    field = ElectricField(x, wavelengths=zc.synthetic_lam(2), spacing=[1e-3, 1e-3], device=_dev())
    with pytest.raises(ValueError, match=r"\[0, 0\)"):
        zc.prop().propagate_zx(field, list(zc.ZS))
