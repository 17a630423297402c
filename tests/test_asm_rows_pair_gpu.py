"""K3 on row pairs (csrc/thz_asm.hip rows_inv_pair_body, csrc/thz_fft.hpp fft_pow2_split2_io): one
workgroup runs output rows 2i and 2i + 1 of a plane through the two-line transform, which pays the
thread-index-only work (twiddle reads, LDS addresses, band and crop tests, barriers) once per pair.

Both forms run the same butterflies through the same helpers (the complex products are written-out
fmaf), so the planes must be BIT-identical to the one-row kernel's: torch.equal, no tolerance.
thz_asm_row_pairs(0 / 1) selects the form per call; K1 and K2 are the same code in both runs.

Shapes: the smallest at which the pair form takes each of its paths, white complex input at cfg2's
sampling (dx 0.25 mm at 300 GHz: the evanescent cut sits inside the padded spectrum, so the band
edge carries energy).
  A  asm_rows_inv_pair<8192, true>, the default of the middle-half crop: 2 planes x (B C = 2)
  B  the generic body at 1024 points, crop [192, 832), Hout = 75 (the one-row tail workgroup of each
     plane, and pairs that would straddle a plane if the tail were not masked), 3 planes
  C  2048 points (three table entries per thread in the fill), even Hout, z_chunk 2 of 3 planes (zoff != 0)
Shape B also against the fp64 oracle with tests/test_asm_gpu.py's rule: rel-L2 <= max(1e-4, 1.5 x the
fp32 oracle's own error on that plane).
"""
import pytest
import torch

from oracle import thz_oracle as orc
from tests.golden_io import rel_l2

pytestmark = pytest.mark.gpu
C0 = 2.998e8


def _both_forms(x, lam, sp, zs, s, **kw):
    from quantizationawarethzdoe_amd import _lib
    from quantizationawarethzdoe_amd.propagation import asm_apply
    H, W = x.shape[-2:]
    ph, pw, _, _ = orc.asm_padding(H, W, s, True)
    outs = []
    try:
        for mode in (0, 1):
            _lib.asm_row_pairs(mode)
            outs.append(asm_apply(x, lam, sp, zs, ph, pw, True, 1, **kw))
            torch.cuda.synchronize()
    finally:
        _lib.asm_row_pairs(-1)
    return outs


def _white(shape, seed):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(*shape, dtype=torch.complex64, device=dev, generator=g)
    lam = [float(torch.tensor(C0 / 300e9, dtype=torch.float32))]
    sp = [float(torch.tensor(0.25e-3, dtype=torch.float32))] * 2
    return x, lam, sp


def _assert_bit_identical(one, two):
    assert one.shape == two.shape
    assert bool(torch.isfinite(torch.view_as_real(two)).all())
    assert float(two.abs().amax()) > 0
    a, b = torch.view_as_real(one), torch.view_as_real(two)
    assert torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} floats differ"


def test_pair_mid_8192_bit_identical_to_one_row():
    """A: Pw = 8192 with the middle-half crop (the kernel cfg2 runs), Ph = 1024, Hout = 512."""
    x, lam, sp = _white((2, 1, 512, 4096), 11)
    one, two = _both_forms(x, lam, sp, [0.02, 0.07], 1)
    assert two.shape == (2, 2, 1, 512, 4096)
    _assert_bit_identical(one, two)


def test_pair_default_is_the_pair_form_at_8192_mid():
    """The library's own choice at A's geometry gives the same planes as either forced form."""
    from quantizationawarethzdoe_amd.propagation import asm_apply
    x, lam, sp = _white((1, 1, 512, 4096), 12)
    one, two = _both_forms(x, lam, sp, [0.05], 1)
    dflt = asm_apply(x, lam, sp, [0.05], 256, 2048, True, 1)
    assert torch.equal(torch.view_as_real(dflt), torch.view_as_real(two))
    assert torch.equal(torch.view_as_real(dflt), torch.view_as_real(one))


def test_pair_generic_1024_odd_rows_bit_identical_and_vs_oracle():
    """B: Pw = 1024 = 640 + 2 x 192 (padding scale 0.6), Hout = 75 (odd), 3 planes."""
    x, lam, sp = _white((1, 1, 75, 640), 13)
    zs = [0.02, 0.05, 0.11]
    assert orc.asm_padding(75, 640, 0.6, True)[3] == 1024
    one, two = _both_forms(x, lam, sp, zs, 0.6)
    assert two.shape == (3, 1, 1, 75, 640)
    _assert_bit_identical(one, two)
    xt = x.cpu()
    lt = torch.tensor(lam, dtype=torch.float32)
    st = torch.tensor(sp, dtype=torch.float32)
    for k, z in enumerate(zs):
        with torch.no_grad():
            r64 = orc.asm_forward(xt.to(torch.complex128), lt.double(), st.double(), z, 0.6).numpy()
            r32 = orc.asm_forward(xt, lt, st, z, 0.6).numpy()
        floor = rel_l2(r32, r64)
        e = rel_l2(two[k].cpu().numpy(), r64)
        print(f"plane {k} z={z}: rel-L2 vs fp64 oracle {e:.3e}, fp32 oracle's own {floor:.3e}")
        assert e <= max(1e-4, 1.5 * floor), (k, z, e, floor)


def test_pair_2048_z_chunks_bit_identical():
    """C: Pw = 2048, Hout = 64, three planes in z-chunks of two (the second launch has zoff = 2)."""
    x, lam, sp = _white((1, 2, 64, 1024), 14)
    lam = lam + [float(torch.tensor(C0 / 280e9, dtype=torch.float32))]
    one, two = _both_forms(x, lam, sp, [0.03, 0.06, 0.09], 1, z_chunk=2)
    assert two.shape == (3, 1, 2, 64, 1024)
    _assert_bit_identical(one, two)


def test_row_pairs_mode_is_validated():
    from quantizationawarethzdoe_amd import _lib
    assert _lib.lib().thz_asm_row_pairs(2) == _lib.THZ_E_ARG
    assert b"thz_asm_row_pairs" in _lib.lib().thz_last_error()
    _lib.asm_row_pairs(-1)
