"""The one property of the shared z-x slice driver (propagation._slice_sweep) that belongs to no
kernel: its two arms agree.  At Z = THZ_MAX_Z + 1 both take two chunks; under ``no_grad`` the whole
[Z, ...] result is allocated once and each chunk's launch writes its part of it, while an input that
requires grad with ``grad="slice"`` goes through the autograd Function per chunk and ``torch.cat``.
The launches are the same, so the results are compared with ``torch.equal`` (two native calls are
bit-identical: test_two_*_calls_are_bit_identical in the three families' own tests).

Shapes: ASM a [1,1,512,64] field with padding scale 1 (padded height 1024, the smallest the slice
kernels serve), and for ``axis="y"`` the square [1,1,512,512] (the padded width must be served too, and
the band limit asks for a square padded plane); CZT GEOMETRIES[3] of tests/test_czt_zx_gpu.py (dx = dy);
RSC / VRS the 20 x 24 geometry of tests/test_rsc_zx_gpu.py.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
CASES = ["asm-x", "asm-y", "czt-x", "czt-y", "rsc-x", "vrs-y"]


def _sweep():
    from quantizationawarethzdoe_amd import _lib
    Z = _lib.THZ_MAX_Z + 1
    return [0.03 + 0.06 * (k / (Z - 1)) ** 1.5 for k in range(Z)]


def case(name, dtype=torch.complex64):
    """(propagator, field data on the device, data -> ElectricField, propagate_zx keywords)."""
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    from quantizationawarethzdoe_amd.Props.ASM_Prop import ASM_prop
    from quantizationawarethzdoe_amd.Props.CZT_Prop import CZT_prop
    from quantizationawarethzdoe_amd.Props.RSC_Prop import RSC_prop, VRS_prop
    dev = torch.device("cuda:0")
    fam, axis = name.split("-")
    kw = dict(axis=axis)
    if fam == "asm":
        shape, dx = (1, 1, 512, 64 if axis == "x" else 512), 0.25e-3
        prop = ASM_prop(z_distance=0.02, padding_scale=1, device=dev)
        prop.check_Zc = False
    elif fam == "czt":
        shape, dx = (2, 1, 20, 24), 0.5e-3
        prop = CZT_prop(z_distance=0.05, device=dev)
        kw.update(outputHeight=20, outputWidth=20, outputPixel_dx=0.2e-3, outputPixel_dy=0.2e-3)
    else:
        shape, dx = (2 if fam == "vrs" else 1, 1, 20, 24), 0.5e-3
        prop = (VRS_prop if fam == "vrs" else RSC_prop)(z_distance=0.05, device=dev)
        prop.check_Zc = False
    g = torch.Generator().manual_seed(1000 * shape[-2] + shape[-1])
    data = torch.randn(*shape, dtype=torch.complex128, generator=g).to(dtype).to(dev)
    wl = torch.tensor([1e-3], dtype=torch.float64) if dtype == torch.complex128 else 1e-3

    def field(x):
        return ElectricField(x, wavelengths=wl, spacing=[dx, dx], device=dev)

    return prop, data, field, kw


@pytest.mark.parametrize("name", CASES)
def test_the_two_arms_of_the_driver_agree(name):
    prop, data, field, kw = case(name)
    zs = _sweep()
    with torch.no_grad():
        whole = prop.propagate_zx(field(data), zs, **kw)
    chunks = prop.propagate_zx(field(data.clone().requires_grad_(True)), zs, grad="slice", **kw)
    assert whole.grad_fn is None and chunks.grad_fn is not None
    assert whole.shape[0] == len(zs) and whole.dtype == torch.complex64
    assert float(whole.abs().flatten(1).amax(1).min()) > 0  # every plane of both chunks was written
    assert torch.equal(torch.view_as_real(whole), torch.view_as_real(chunks.detach()))
