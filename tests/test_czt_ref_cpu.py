"""tests/czt_ref.py pinned before it judges a kernel (no GPU).

* ``grids="fp64"`` in complex128 is oracle.thz_oracle.czt_forward under a float64 default dtype, and
  its autograd adjoint the oracle's, to 1e-12 relative L2, on every entry of the parity matrix below
  300 in both axes (both geometries) and on one overlap-add-sized entry.
* ``grids="fp32"`` rests on czt_ref.lin32, float32 ``torch.linspace`` element by element (start + step
  i in the lower half, end - step (n - 1 - i) in the upper, step = (end - start) / (n - 1), every
  operation in float32 -- what the kernels' ``lin()`` restates): compared bit for bit with that
  definition in numpy float32 scalars at every length of the matrix, antisymmetric to the bit, and
  within one ulp of torch's chunked CPU linspace (which is NOT bit-equal to it: 1536 points at 0.02 mm).
* floor32 -- the complex64 run against the complex128 run, per plane, both metrics -- is positive and
  below 1e-5 on every entry of the matrix: the condition that keeps MARGIN x floor32 a tight bound.
* The phase term PH of the bound, from the geometry alone: in the tight geometry it stays under 2.5e-6
  (its whole bound under 1e-5); in the physical geometry it exceeds MARGIN x floor32 on every entry
  whose field is longer than 1000 pixels (the RS factors decide there).
"""
import numpy as np
import pytest
import torch

from oracle import thz_oracle as orc
from tests import czt_ref as cr

TOL = 1e-12
SMALL = [r for r in cr.ROWS if max(r[0], r[1]) < 300]
PINNED = [(r, g) for r in SMALL for g in cr.GEOMETRIES] + [(cr.ROWS[5], "physical")]
ALL = [(r, g) for r in cr.ROWS for g in cr.GEOMETRIES]


def _id(v):
    return cr.row_id(v) if isinstance(v, tuple) else v


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def _oracle(x, row, geo, g=None):
    """orc.czt_forward in fp64 (and its autograd adjoint of g) on the launch's float32-rounded values"""
    H, W, M, B, C = row[:5]
    dx, dy, odx, ody, z = (cr.f32(v) for v in cr.GEOMETRIES[geo])
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        xo = x.to(cr.C128).requires_grad_(g is not None)
        out = orc.czt_forward(xo, torch.tensor(cr.wavelengths(C), dtype=torch.float64),
                              torch.tensor([dx, dy], dtype=torch.float64), z, M, M, odx, ody)
        if g is None:
            return out
        gin, = torch.autograd.grad(out, xo, grad_outputs=g.to(cr.C128))
        return out.detach(), gin
    finally:
        torch.set_default_dtype(prev)


@pytest.mark.parametrize("row, geo", PINNED, ids=_id)
def test_fp64_grids_in_complex128_is_the_oracle(row, geo):
    case, x, g = cr.build(row, geo, grids="fp64")
    want, want_g = _oracle(x, row, geo, g)
    got, got_g = case.grad(x, g)
    assert got.shape == want.shape == (row[3], row[4], row[2], row[2])
    assert _rel(got, want) <= TOL and _rel(got_g, want_g) <= TOL, (_rel(got, want), _rel(got_g, want_g))


def test_float32_grid_is_the_elementwise_linspace():
    for geo, (dx, dy, odx, ody, _) in cr.GEOMETRIES.items():
        for n, d in sorted({(r[0], dx) for r in cr.ROWS} | {(r[1], dy) for r in cr.ROWS} | {(r[2], odx) for r in cr.ROWS}
                           | {(r[2], ody) for r in cr.ROWS}):
            e = n * cr.f32(d) / 2
            got = cr.lin32(-e, e, n)
            assert got.dtype == torch.float32 and got.shape == (n,)
            # the definition, element by element in numpy float32 scalars
            s, t = np.float32(-e), np.float32(e)
            step = (t - s) / np.float32(max(n - 1, 1))
            want = [s + step * np.float32(i) if i < n // 2 or n == 1 else t - step * np.float32(n - 1 - i)
                    for i in range(n)]
            assert np.array_equal(got.numpy(), np.array(want, dtype=np.float32)), (geo, n, d)
            # two-sided: antisymmetric to the bit; within an ulp of torch's chunked CPU kernel and within
            # n / 2 roundings of the end value of the float64 grid
            assert torch.equal(got[:n // 2], -got.flip(0)[:n // 2])   # (an odd n's centre comes from the upper end)
            ulp = float(np.spacing(np.float32(e)))
            assert float((got - torch.linspace(-e, e, n, dtype=torch.float32)).abs().max()) <= ulp
            assert float((got.double() - torch.linspace(-e, e, n, dtype=torch.float64)).abs().max()) <= n / 2 * ulp


def test_matrix_forms_follow_the_cost_rule():
    """The form each row claims for its passes is what the restated make_pass rule gives (the GPU test
    asserts it again from the launch counts), no Bluestein length is a power of two, no shape exceeds
    2100 and no call six planes."""
    for H, W, M, B, C, fa, fb in cr.ROWS:
        assert (cr.pass_form(W, M), cr.pass_form(H, M)) == (fa, fb), (H, W, M)
        assert all(n & (n - 1) for n in (H + M - 1, W + M - 1)) and max(H, W) <= 2100 and B * C <= 6
    assert (cr.pass_form(1536, 17), cr.pass_form(1537, 17)) == (cr.BLK, cr.NP2)   # the cost switch
    assert (cr.pass_form(1536, 512), cr.pass_form(1100, 513)) == (cr.BLK, cr.NP2)  # the M cap


@pytest.mark.parametrize("row, geo", ALL, ids=_id)
def test_floor32_and_phase_term(row, geo):
    H, W, M, B, C, fa, fb = row
    case, x, _ = cr.build(row, geo)
    ref, lo = case.forward(x), case.forward(x, cr.C64)
    assert lo.dtype == cr.C64
    for b in range(B):
        for c in range(C):
            floor = cr.floor_of(lo[b, c], ref[b, c])   # asserts 0 < floor32 < 1e-5 on both metrics
            ph = cr.phase_term(case, c, fa, fb)
            if geo == "tight":
                assert ph < 2.5e-6 and max(cr.bound(floor, ph)) < 1e-5, (floor, ph)
            elif max(H, W) > 1000:
                assert ph > cr.MARGIN * floor[1], (floor, ph)
