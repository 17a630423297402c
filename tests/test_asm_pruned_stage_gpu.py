"""The half-empty first stage of the column pass's inverse transform (csrc/thz_fft.hpp
dft16<INV, false, MID_IN>, taken by asm_cols on its wave-uniform mid0 flag): where a column's kept band
stays below P/4, the radix-16 first stage's operands 4..11 are zero for every thread and the stage
runs without them; a band that reaches P/4 runs the full stage.  The row pass (asm_rows_inv) skips
only the loads of its zero operands and keeps the full stage (the pruned one measured slower there,
DESIGN.md section 16); the same cases cover its load skip on both sides of the boundary.

Geometry: P = 1024, the smallest instantiated power-of-two size (Pow2Sizes in csrc/thz_launch.hpp; its
inverse schedules are 16 x 16 x 4, radix 16 first, in both the column and the row pass).  Padding scale 1
makes P = 2 N, so both passes reach that size only with a 512 x 512 field (a smaller field runs the
runtime plans, which have no such stage).  White-noise inputs: the band edge carries energy.

Tolerances.  Against the fp64 oracle each plane's rel-L2 is <= max(1e-4, 1.5 x the fp32 oracle's own
error on it), the rule of tests/test_asm_gpu.py (test_asm_multi_z_matches_oracle).  The adjoint identity
is held to |<A x, g> - <x, A^H g>| <= 1e-5 ||A x|| ||g||, the bound tests/test_properties_gpu.py uses for
these kernels (test_asm_pow2_columns_linearity_and_adjoint).

Pruned == full.  The pruned stage keeps the full butterfly's surviving sums in their order, so on the
same data both give the same bits up to the sign of a zero.  For the column pass no pair of runs that
takes one stage each on the same data can be built through the public API: its flag is the column's
own kept-row bound M < P/4, a function of the transfer function alone, so every setting that lifts M
to P/4 (a shorter wavelength, a coarser grid, band limit off -- which multiplies the padded field's
out-of-band spectrum by a non-zero H instead of zero) changes the math.  Its two stages are graded by
the oracle legs only.  For the row pass the pair exists and is kept (its zero operands skipped against
loaded as explicit zeros): the kept column band J is the widest over the call's wavelengths, so a
second, short wavelength in the same call widens J past P/4 and the long wavelength's rows gather
columns that the column pass filled with exact zeros -- compared with torch.equal.
"""
import os

import numpy as np
import pytest
import torch

from oracle import thz_oracle as orc
from tests.golden_io import rel_l2

pytestmark = pytest.mark.gpu
C0 = 2.998e8
N, PAD, P = 512, 256, 1024
DX = float(np.float32(0.25e-3))
UNIFORM4 = [0.05 + 0.004 * k for k in range(4)]   # a uniform sweep
NONUNIFORM3 = [0.02, 0.05, 0.11]                  # the column pass's per-plane sincos form
# A sweep long enough for the plane recurrence at this size: the 407 band columns are fewer than the
# column workgroups one dispatch round holds (at most 16 per CU), so the column pass splits the planes
# into up to 10 z-ranges per column (k2_tasks) and a range under 3 planes keeps the sincos form --
# as the 4-plane sweep does here.  48 planes leave every range 4 or more.
UNIFORM48 = [0.03 + 0.002 * k for k in range(48)]
_X = {}


def _f32(v):
    return float(np.float32(v))


def _field(seed, shape=(1, 1, N, N)):
    """White complex noise from a seeded host generator (cached: the tests share the inputs)."""
    key = (seed, shape)
    if key not in _X:
        g = torch.Generator().manual_seed(seed)
        _X[key] = torch.randn(*shape, dtype=torch.complex64, generator=g)
    return _X[key]


def _ncols(lam, dx, zs):
    from quantizationawarethzdoe_amd.propagation import asm_plan_info
    return asm_plan_info(1, len(lam), N, N, PAD, PAD, True, 1, lam, [dx, dx], zs)[0]


def _apply(x, lam, dx, zs, **kw):
    from quantizationawarethzdoe_amd.propagation import asm_apply
    out = asm_apply(x.to("cuda:0"), lam, [dx, dx], zs, PAD, PAD, True, 1, **kw)
    torch.cuda.synchronize()
    return out


def _grade(out, x, lam, dx, zs, planes=None):
    """The planes (default: all) against the fp64 oracle, at max(1e-4, 1.5 x the fp32 oracle's own error)."""
    lt = torch.tensor(lam, dtype=torch.float32)
    st = torch.tensor([dx, dx], dtype=torch.float32)
    planes = list(range(len(zs))) if planes is None else planes
    zp = [zs[k] for k in planes]
    with torch.no_grad():
        r64 = list(orc.asm_forward_planes(x.to(torch.complex128), lt.double(), st.double(), zp, 1))
        r32 = list(orc.asm_forward_planes(x, lt, st, zp, 1))
    for k, (_, p64), (_, p32) in zip(planes, r64, r32):
        floor = rel_l2(p32.numpy(), p64.numpy())
        e = rel_l2(out[k].cpu().numpy(), p64.numpy())
        print(f"plane {k} z {zs[k]:.4f}: rel-L2 {e:.3e} (fp32 oracle {floor:.3e})")
        assert e <= max(1e-4, 1.5 * floor), (k, zs[k], e, floor)


def _lam_for_ncols(target, zs):
    """A wavelength at which the plan keeps `target` columns: the band half-width follows P dx / lam."""
    for q in np.arange(248.0, 272.0, 0.05):
        lam = [_f32(P * DX / q)]
        if _ncols(lam, DX, zs) == target:
            return lam
    raise AssertionError(f"no wavelength gives ncols == {target}")


@pytest.mark.parametrize("zs", [UNIFORM4, NONUNIFORM3, UNIFORM48],
                         ids=["uniform4", "nonuniform3_sincos", "uniform48_recurrence"])
def test_narrow_band_pruned_stage_vs_oracle(zs):
    """240 GHz at dx 0.25 mm: the evanescent cut sits at |m| ~ 205 of P/4 = 256, so every column takes the
    pruned stage, in the column pass's sincos form (the short lists) and in its recurrence form (the
    48-plane sweep: every 5th plane and each end graded)."""
    lam = [_f32(C0 / 240e9)]
    ncols = _ncols(lam, DX, zs)
    assert ncols <= 2 * (P // 4 - 32) + 1, ncols
    x = _field(11)
    out = _apply(x, lam, DX, zs)
    if zs is UNIFORM48:
        # the recurrence really ran: the per-plane sincos form of the same kernel differs from it
        old = os.environ.get("THZ_K2_RECURRENCE")
        os.environ["THZ_K2_RECURRENCE"] = "0"
        try:
            sincos = _apply(x, lam, DX, zs)
        finally:
            if old is None:
                del os.environ["THZ_K2_RECURRENCE"]
            else:
                os.environ["THZ_K2_RECURRENCE"] = old
        assert not torch.equal(out, sincos)
        _grade(out, x, lam, DX, zs, sorted(set(range(0, len(zs), 5)) | {1, len(zs) - 1}))
        return
    _grade(out, x, lam, DX, zs)


@pytest.mark.parametrize("J", [P // 4 - 1, P // 4], ids=["J_quarter_minus_1", "J_quarter"])
def test_band_at_the_quarter_boundary_vs_oracle(J):
    """J = P/4 - 1 is the widest band at which every wave of the row pass skips its operands 4..11; at
    J = P/4 the wave that straddles the boundary gathers them.  The column pass keeps |m_x| <= J - 2: pruned."""
    zs = UNIFORM4
    lam = _lam_for_ncols(2 * J + 1, zs)
    x = _field(12)
    _grade(_apply(x, lam, DX, zs), x, lam, DX, zs)


def test_wide_band_full_stage_vs_oracle():
    """dx 1 mm at 300 GHz: the band passes P/4 in every column, so the column pass runs the full stage."""
    dx = _f32(1e-3)
    lam = [_f32(C0 / 300e9)]
    zs = UNIFORM4
    assert _ncols(lam, dx, zs) > 2 * (P // 4 + 32) + 1
    x = _field(13)
    _grade(_apply(x, lam, dx, zs), x, lam, dx, zs)


def test_row_pass_pruned_equals_full_on_the_same_data():
    """The long wavelength alone (narrow J: the row pass skips its zero operands) against the same field in
    a call whose second, short wavelength widens J (the row pass gathers them as explicit zeros): equal,
    0 == -0 included."""
    zs = NONUNIFORM3
    lam = [_f32(C0 / 240e9), _f32(C0 / 600e9)]
    assert _ncols(lam[:1], DX, zs) <= 2 * (P // 4 - 32) + 1
    assert _ncols(lam, DX, zs) > 2 * (P // 4 + 32) + 1
    x2 = _field(14, (1, 2, N, N))
    pruned = _apply(x2[:, :1].contiguous(), lam[:1], DX, zs)
    full = _apply(x2, lam, DX, zs)[:, :, :1]
    assert pruned.abs().amax() > 0
    diff = float((pruned - full).abs().amax())
    print(f"max |pruned - full| = {diff:.3e}")
    assert torch.equal(pruned, full), diff


def test_adjoint_identity_on_the_pruned_path():
    """<A x, g> = <x, A^H g> on the narrow band: through autograd for one plane (the single-plane column
    pass, pruned, in both directions) and for the Z-summing adjoint launch of a sweep (the shared row
    pass)."""
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    from quantizationawarethzdoe_amd.Props.ASM_Prop import ASM_prop
    dev = torch.device("cuda:0")
    lam = [_f32(C0 / 240e9)]
    x = _field(15).to(dev)

    def check(Ax, g, AHg):
        lhs = torch.vdot(Ax.reshape(-1).to(torch.complex128), g.reshape(-1).to(torch.complex128))
        rhs = torch.vdot(x.reshape(-1).to(torch.complex128), AHg.reshape(-1).to(torch.complex128))
        bound = 1e-5 * float(Ax.norm()) * float(g.norm())
        print(f"|<Ax,g> - <x,AHg>| = {abs(complex(lhs - rhs)):.3e} (bound {bound:.3e})")
        assert abs(complex(lhs - rhs)) <= bound

    xg = x.clone().requires_grad_(True)
    prop = ASM_prop(z_distance=0.05, padding_scale=1, bandlimit_type="exact", device=dev)
    out = prop(ElectricField(xg, wavelengths=lam[0], spacing=DX, device=dev)).data
    g1 = _field(16).to(dev)
    gx, = torch.autograd.grad(out, xg, grad_outputs=g1)
    check(out.detach(), g1, gx)

    zs = UNIFORM4
    Ax = _apply(x, lam, DX, zs)
    g = _field(17, (len(zs), 1, 1, N, N)).to(dev)
    check(Ax, g, _apply(g, lam, DX, zs, adjoint=True))
