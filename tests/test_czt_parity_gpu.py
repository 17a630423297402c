"""CZT parity: CZT_prop's kernels against an fp64 reference on the float32 grid values, per plane.

Every other fp32 value check of the chirp-z propagator is a relative L2 of 1e-3 or 3e-3 over a whole
call (tests/test_czt_gpu.py, bench.check_czt): three orders above what the build does -- chirps formed
in double, the RS phase as kz mod 2 pi + k rho^2 / (r + |z|) -- so a wrong element at a 512-input
block seam, a chirp off by 1e-4 or one wrong post[] entry passes them.  The CZT exports no table, so
the reference here is tests/czt_ref.py (pinned by tests/test_czt_ref_cpu.py): the reference's algebra in
complex128 on the float32 coordinate grids the kernels' lin() forms, forward and, by autograd, adjoint.

Input and grad_output are seeded complex white noise.  Every (b, c) plane is judged on its own -- a
wrong wavelength index or plane stride cannot hide -- on two metrics: relative L2, and max|err| /
rms(ref), the one a single wrong element of a large plane cannot hide in.

Bound, on both: err <= MARGIN x floor32 + PH.
* floor32: the same algebra with every factor and table rounded once to complex64 and a complex64 data
  path on torch's CPU FFT, against the complex128 run, for that plane (forward) or through its own
  autograd (backward): 0.4e-7 ... 1e-6 rel-L2, up to 1.4e-6 max/rms on this matrix.  MARGIN = 4 is
  tests/test_table_parity_gpu.py's constant and argument: a different but equally valid fp32 FFT.
* PH = c 2^-24 max(k rho^2 / (r + |z|)) over the input and the output mesh of the plane's wavelength:
  the kernels round the residual RS phase in fp32.  c counts the fp32 roundings on the way to the
  argument of the sine and cosine in csrc/thz_dev.hpp.  rs_kernel: x x, y y, their sum, z z, rho2 + z z,
  sqrtf, r + |z|, the division, the product with k, the sum with kzmod -- 10 operations -- and the two
  constants k and kzmod rounded from double: c = 12.  rs_kernel_fast (the overlap-add kernels): 12
  operations, of which the hardware rsq (one ulp) counts twice and the Newton-refined rcp as its two
  fused steps, and the two constants: c = 16.  Each mesh takes the c of the function its pass
  evaluates (pass A the input mesh, pass B the output mesh; the adjoint runs rs_kernel on both).  c is
  counted from the code, not fitted: measured ratios are in profiles/czt_parity_ratios.txt.  Not in
  PH: the absolute error of the sine / cosine themselves (sincos_rad 6e-8, sincos_hw 1.8e-7), the
  amplitude's few roundings and cis_d's fp32 evaluation of the chirps; they are of the size of one
  complex64 rounding per factor, which floor32 also pays, and MARGIN has to absorb them.
* A plane of one or two elements (M = 1, M = 2) can land its complex64 run under one rounding by
  chance; each floor32 figure is taken as at least 2^-24 (czt_ref.floor_of), so the M = 1 rows are
  judged at no less than 4 x 2^-24 + PH.

Two geometries per shape (czt_ref.GEOMETRIES).  "tight": 0.02 mm pixels in, 0.03 / 0.025 mm out, z =
0.5 m: the residual phase stays under 3.2 rad, PH under 2.3e-6 and the whole bound under 1e-5, so
seams, tables, chirps and stores are judged at 1e-6.  "physical": 0.5 / 0.6 mm in, 0.35 / 0.3 mm out,
z = 0.2 m: phases up to 2.6e3 rad, PH decides; the RS factors of both meshes with dy != dx and ody !=
odx.  Wavelengths 300 / 340 / 380 GHz.

Every shape asserts the form (np2 pair or overlap-add) make_pass gives each pass, read from the launch
counts of csrc/thz_czt.hip's timers czt_rows / czt_rows_blk / czt_cols / czt_cols_blk / czt_adjoint.

Each case prints its lines (worst plane per metric); THZ_CZT_PARITY_LOG=<file> appends them to a file.
"""
import os

import pytest
import torch

from tests import czt_ref as cr

pytestmark = pytest.mark.gpu
TIMERS = ("czt_rows", "czt_rows_blk", "czt_cols", "czt_cols_blk", "czt_adjoint")
CASES = [(r, g) for r in cr.ROWS for g in cr.GEOMETRIES]


def _id(v):
    return cr.row_id(v) if isinstance(v, tuple) else v


def _dev():
    return torch.device("cuda:0")


def _launches(fn):
    """(result of fn(), launches of each timer of TIMERS)"""
    from quantizationawarethzdoe_amd import _lib
    _lib.timing_enable(True)
    try:
        _lib.timing_reset()
        out = fn()
        return out, tuple(_lib.timing_read(n)[1] for n in TIMERS)
    finally:
        _lib.timing_enable(False)


def _judge(what, name, got, ref, lo, ph):
    """The (b, c) planes of ``got`` against ``ref`` with ``lo`` the complex64 run; ph[c] the phase term.
    One line per metric (its worst plane), then the assertion on every plane."""
    B, C = ref.shape[:2]
    assert got.shape == ref.shape and got.dtype == cr.C64
    worst = [None, None]
    for b in range(B):
        for c in range(C):
            err = cr.errors(got[b, c], ref[b, c])
            floor = cr.floor_of(lo[b, c], ref[b, c])
            bnd = cr.bound(floor, ph[c])
            for k in range(2):
                rec = (err[k] / bnd[k], b, c, floor[k], ph[c], err[k], bnd[k])
                if worst[k] is None or rec[0] > worst[k][0]:
                    worst[k] = rec
    lines = []
    for k, metric in enumerate(("rel-L2", "max/rms")):
        ratio, b, c, fl, p, e, bn = worst[k]
        lines.append(f"czt-parity {what:<8s} {name:<32s} {metric:<7s} worst plane b{b} c{c}  floor32 {fl:.3e}  PH {p:.3e}"
                     f"  err {e:.3e}  bound {bn:.3e}  err/bound {ratio:5.3f}")
    for line in lines:
        print(line)
    log = os.environ.get("THZ_CZT_PARITY_LOG")
    if log:
        with open(log, "a") as f:
            f.write("".join(line + "\n" for line in lines))
    assert worst[0][0] <= 1 and worst[1][0] <= 1, "\n".join(lines)


def _field(x, C, geo, dtype=cr.C64):
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    dx, dy = cr.GEOMETRIES[geo][:2]
    wl = cr.wavelengths(C)
    if dtype == cr.C128:
        wl = torch.tensor(wl, dtype=torch.float64)
    elif C == 1:
        wl = wl[0]
    return ElectricField(x, wavelengths=wl, spacing=[dx, dy], device=_dev())


def _prop(field, M, geo):
    from quantizationawarethzdoe_amd.Props.CZT_Prop import CZT_prop
    _, _, odx, ody, z = cr.GEOMETRIES[geo]
    return CZT_prop(z_distance=z, device=_dev())(field, M, M, odx, ody).data


@pytest.mark.parametrize("row, geo", CASES, ids=_id)
def test_czt_forward_and_backward(row, geo):
    H, W, M, B, C, fa, fb = row
    assert all(n & (n - 1) for n in (H + M - 1, W + M - 1))
    case, x, g = cr.build(row, geo)
    name = f"{cr.row_id(row)} {geo}"
    xd = x.to(_dev()).requires_grad_(True)
    out, n = _launches(lambda: _prop(_field(xd, C, geo), M, geo))
    # the form each pass took: one launch per pass, the overlap-add ones also under their own names
    assert n == (1, int(fa == cr.BLK), 1, int(fb == cr.BLK), 0), (n, fa, fb)
    gin, n = _launches(lambda: torch.autograd.grad(out, xd, grad_outputs=g.to(_dev()))[0])
    assert n == (0, 0, 0, 0, 1), n   # the adjoint: the np2 kernels whatever the forward took
    ref, ref_g = case.grad(x, g)
    lo, lo_g = case.grad(x, g, cr.C64)
    _judge("forward", name, out.detach().cpu(), ref, lo, [cr.phase_term(case, c, fa, fb) for c in range(C)])
    _judge("backward", name, gin.cpu(), ref_g, lo_g, [cr.phase_term(case, c, cr.NP2, cr.NP2) for c in range(C)])


@pytest.mark.parametrize("row", [(37, 53, 15), (37, 53, 1), (200, 1100, 24), (1030, 1030, 2)],
                         ids=lambda r: f"{r[0]}x{r[1]}_M{r[2]}")
@pytest.mark.parametrize("geo", list(cr.GEOMETRIES))
def test_czt_complex128_entry_per_plane(row, geo):
    """The complex128 path (thz_czt64_forward: complex128 data, float64 wavelengths) with B x C = 2 x 2
    against the truth on float64 grids, every plane within tests/test_f64_gpu.py's 1e-8 rel-L2.  That
    entry takes the output pixels and z as the doubles they are (only the field's spacing and the
    wavelengths are float32 values), and so does the truth here (as_given).  max|err| / rms(ref) is held
    to 5e-8: errors of an rms within the 1e-8 peak below five times that over planes of up to 576
    elements (Gaussian tail: sqrt(2 ln n) < 3.6), so one wrong element cannot hide in the L2."""
    H, W, M = row
    full = (H, W, M, 2, 2, cr.NP2, cr.NP2)
    case, x, _ = cr.build(full, geo, grids="fp64", as_given=True)
    out = _prop(_field(x.to(cr.C128).to(_dev()), 2, geo, cr.C128), M, geo).cpu()
    ref = case.forward(x)
    assert out.dtype == cr.C128 and out.shape == ref.shape
    for b in range(2):
        for c in range(2):
            rel, mx = cr.errors(out[b, c], ref[b, c])
            print(f"czt-parity c128     {H}x{W}_M{M} {geo} b{b} c{c} rel-L2 {rel:.3e} max/rms {mx:.3e}")
            assert rel <= 1e-8 and mx <= 5e-8, (b, c, rel, mx)
