"""tests/table_ref.py pinned before it judges a kernel: fed the oracle's own fp64 table it reproduces
oracle.thz_oracle.asm_forward / rsc_forward, and their autograd adjoints, to 1e-12 relative L2 (fp64
round-off of a different but equal op order: one shared spectrum, the planes summed before the inverse
transform).  Geometries: odd sizes, padding scale 1.5, unpad=False, do_padding=False, H != W, C = 2.
"""
import pytest
import torch

from oracle import thz_oracle as orc
from tests import table_ref as tr

TOL = 1e-12
C0 = 2.998e8
LAM2 = torch.tensor([C0 / 280e9, C0 / 320e9], dtype=torch.float64)

# (B, C, H, W, padding_scale, do_padding, unpad, bandlimit, bandlimit_type, (dx, dy), z)
ASM_CASES = [
    (1, 1, 32, 32, 1, True, True, True, "exact", (0.5e-3, 0.5e-3), 0.02),
    (2, 2, 33, 47, 1, True, True, True, "exact", (0.5e-3, 0.4e-3), 0.03),          # odd, H != W, C = B = 2
    (1, 2, 20, 28, 1.5, True, True, True, "approx", (0.5e-3, 0.5e-3), 0.015),      # padding scale 1.5
    (1, 1, 21, 30, 1.5, True, False, True, "exact", (0.5e-3, 0.5e-3), 0.02),       # unpad=False, odd pad
    (1, 2, 36, 25, 1, False, True, False, "exact", (0.5e-3, 0.5e-3), -0.04),       # do_padding=False, no band limit
    (1, 1, 24, 40, (2, 1), True, True, False, "exact", (0.4e-3, 0.5e-3), 0.05),    # a scale per axis
]


def _white(shape, seed):
    return torch.randn(*shape, dtype=torch.complex128, generator=torch.Generator().manual_seed(seed))


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def _asm_setup(case):
    B, C, H, W, s, pad, unpad, bl, blt, sp, z = case
    lam = LAM2[:C]
    ph, pw, Ph, Pw = orc.asm_padding(H, W, s, pad)
    Hc = orc.asm_transfer_function(Ph, Pw, lam, sp[0], sp[1], z, bl, blt, rdt=torch.float64)
    fwd = lambda x: orc.asm_forward(x, lam, sp, z, s, pad, unpad, bl, blt)
    return lam, ph, pw, Hc, fwd


@pytest.mark.parametrize("case", ASM_CASES, ids=lambda c: f"{c[2]}x{c[3]}_s{c[4]}_{c[8] if c[7] else 'none'}")
def test_asm_from_table_is_the_oracle(case):
    B, C, H, W = case[:4]
    unpad = case[6]
    lam, ph, pw, Hc, fwd = _asm_setup(case)
    assert Hc.dtype == torch.complex128 and float((Hc != 0).double().mean()) > 0.25
    x = _white((B, C, H, W), 7).requires_grad_(True)
    want = fwd(x)
    got = tr.asm_from_table(x.detach(), Hc, ph, pw, unpad)
    assert got.shape == want.shape and got.dtype == torch.complex128
    assert _rel(got, want.detach()) <= TOL
    two = tr.asm_planes_from_tables(x.detach(), [Hc, 2 * Hc], ph, pw, unpad)
    assert torch.equal(two[0], got) and _rel(two[1], 2 * want.detach()) <= TOL
    # the adjoint, three planes: the table of each plane differs by a plane-dependent phase factor
    g = _white((3,) + tuple(want.shape), 8)
    facs = [1.0, torch.exp(torch.tensor(0.7j)), torch.exp(torch.tensor(-1.9j))]
    want_adj = sum(torch.autograd.grad(fwd(x) * f, x, grad_outputs=g[k])[0] for k, f in enumerate(facs))
    got_adj = tr.asm_adjoint_from_table(g, [Hc * f for f in facs], ph, pw, unpad)
    assert got_adj.shape == x.shape
    assert _rel(got_adj, want_adj) <= TOL


def _rs_table64(H, W, lam, dx, z):
    """the K oracle.thz_oracle.rsc_forward forms, in fp64"""
    Ph, Pw = H + 2 * (H // 2), W + 2 * (W // 2)
    x = torch.linspace(-Ph * dx / 2, Ph * dx / 2, Ph, dtype=torch.float64)
    y = torch.linspace(-Pw * dx / 2, Pw * dx / 2, Pw, dtype=torch.float64)
    mx, my = torch.meshgrid(x, y, indexing="ij")
    return orc._rs_kernel(torch.tensor(z, dtype=torch.float64), mx[None, None], my[None, None], lam)


# (B, C, H, W, (dx, dy), z)
RSC_CASES = [
    (1, 1, 32, 32, (0.25e-3, 0.25e-3), 0.05),
    (1, 2, 33, 47, (0.25e-3, 0.3e-3), 0.03),     # odd, H != W, dx != dy, C = 2
    (1, 2, 20, 25, (0.5e-3, 0.5e-3), 0.0725),
]


@pytest.mark.parametrize("case", RSC_CASES, ids=lambda c: f"{c[2]}x{c[3]}")
def test_rsc_from_table_is_the_oracle(case):
    B, C, H, W, sp, z = case
    lam = torch.tensor([1e-3 * (1 + 0.1 * c) for c in range(C)], dtype=torch.float64)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        x = _white((B, C, H, W), 9).requires_grad_(True)
        want = orc.rsc_forward(x, lam, list(sp), z)
        K = _rs_table64(H, W, lam, sp[0], z)
        got = tr.rsc_from_table(x.detach(), K, sp[0], sp[1])
        assert got.shape == want.shape == (B, C, 2 * (H // 2), 2 * (W // 2))
        assert _rel(got, want.detach()) <= TOL
        g = _white(tuple(want.shape), 10)
        want_adj, = torch.autograd.grad(want, x, grad_outputs=g)
        assert _rel(tr.rsc_adjoint_from_table(g, K, sp[0], sp[1], H, W), want_adj) <= TOL
    finally:
        torch.set_default_dtype(old)


def test_vrs_from_table_is_the_zx_oracle():
    """Ez as tests/test_rsc_zx_gpu._oracle_planes forms it: that file's VRS geometry and sweep."""
    from tests import test_rsc_zx_gpu as zx
    geo = zx.VRS
    H, W, C, B, sp = geo
    want = zx._oracle_planes(geo, zx.ZS, True)
    dx, dy = zx._f32(sp[0]), zx._f32(sp[1])
    lam = torch.tensor([zx._f32(v) for v in zx._lam(C)], dtype=torch.float64)
    x = zx._input(geo)
    for k, z in enumerate(zx.ZS):
        z = zx._f32(z)
        got = tr.vrs_from_table(x, _rs_table64(H, W, lam, dx, z), dx, dy, z)
        assert got.shape == want[k].shape and _rel(got, want[k]) <= TOL
    # the VRS adjoint against autograd through the forward just pinned
    z, K = zx._f32(zx.ZS[0]), _rs_table64(H, W, lam, dx, zx._f32(zx.ZS[0]))
    xg = x.to(torch.complex128).requires_grad_(True)
    y = tr.vrs_from_table(xg, K, dx, dy, z)
    g = _white(tuple(y.shape), 12)
    want_adj, = torch.autograd.grad(y, xg, grad_outputs=g)
    assert _rel(tr.vrs_adjoint_from_table(g, K, dx, dy, z, H, W), want_adj) <= TOL


def test_floor32_and_errors():
    """floor32 is the same algebra in complex64: an fp32 FFT round-off, far above fp64's and far below
    the suite's oracle bounds; errors() gives one wrong element all of the elementwise metric."""
    case = ASM_CASES[1]
    B, C, H, W = case[:4]
    lam, ph, pw, Hc, _ = _asm_setup(case)
    x = _white((B, C, H, W), 11).to(torch.complex64)
    ref = tr.asm_from_table(x, Hc.to(torch.complex64), ph, pw)
    assert ref.dtype == torch.complex128
    rel, mx = tr.floor32(tr.asm_from_table, x, Hc.to(torch.complex64), ph, pw, ref=ref)
    assert (rel, mx) == tr.floor32(tr.asm_from_table, x, Hc.to(torch.complex64), ph, pw)
    assert 1e-8 < rel < 2e-6 and rel < mx < 1e-5
    bad = ref.clone()
    rms = float(ref.abs().pow(2).mean().sqrt())
    bad[0, 0, 3, 5] += 1e-3 * rms
    r2, m2 = tr.errors(bad, ref)
    assert abs(m2 - 1e-3) < 1e-9 and abs(r2 - 1e-3 / ref.numel() ** 0.5) < 1e-9
