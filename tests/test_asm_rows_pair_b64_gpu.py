"""K3 on row pairs, the interleaved two-line image (csrc/thz_fft.hpp fft_pow2_split2_io, pair_lay): both
lines of a pair share one float2 per element, so each exchange part is one 8-byte DS access.  Neither
the schedule nor a butterfly changes, so the pair form stays BIT-identical to the one-row kernel:
torch.equal on the complex64 planes of thz_asm_row_pairs(1) against thz_asm_row_pairs(0), through
asm_apply on seeded white noise (every band element non-zero).

Shapes: every power-of-two size has its own pair_lay constants and exchange count, so each runs once,
at the smallest field that still takes the path in question:
  Pw 1024, Hout = 7 (odd): the tail workgroup of each plane, whose second line transforms zeros and
           must store nothing -- the planes sit in a sentinel-filled buffer one row longer than needed
  Pw 2048, 4096, 16384: Z = 2 planes, B C = 2 (plane / batch indexing of the pair grid), 6 rows
  Pw 8192 at the middle-half crop: asm_rows_inv_pair<8192, true>, the library's default; Z = 2, 4096 rows
  Pw 8192, crop [2096, 6096): asm_rows_inv_pair<8192, false>
and one anchor that does not lean on the one-row form: Pw 1024 with the pair form forced, against
tests/table_ref.py's complex128 algebra on the exported table, under tests/test_table_parity_gpu.py's
rule (both metrics within 4 x the floor of the same algebra run in complex64).
"""
import pytest
import torch

from tests import table_ref as tr
from tests import test_table_parity_gpu as tp

pytestmark = pytest.mark.gpu
C0 = 2.998e8
SENTINEL = complex(-7.25, 3.5)


def _white(shape, seed, channels=1):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(*shape, dtype=torch.complex64, device=dev, generator=g)
    lam = [float(torch.tensor(C0 / (f * 1e9), dtype=torch.float32)) for f in (300, 280)[:channels]]
    sp = [float(torch.tensor(0.25e-3, dtype=torch.float32))] * 2
    return x, lam, sp


def _both_forms(x, lam, sp, zs, ph, pw, extra_rows=0):
    """The planes of the one-row form and of the pair form, each written into a sentinel-filled flat
    buffer with room for ``extra_rows`` more output rows: (planes, what lies behind them) per form."""
    from quantizationawarethzdoe_amd import _lib
    from quantizationawarethzdoe_amd.propagation import asm_apply
    B, C, H, W = x.shape
    shape = (len(zs), B, C, H, W)
    n = len(zs) * B * C * H * W
    res = []
    try:
        for mode in (0, 1):
            _lib.asm_row_pairs(mode)
            buf = torch.full((n + extra_rows * W,), SENTINEL, dtype=torch.complex64, device=x.device)
            asm_apply(x, lam, sp, zs, ph, pw, True, 1, out=buf)
            torch.cuda.synchronize()
            res.append((buf[:n].view(shape), buf[n:]))
    finally:
        _lib.asm_row_pairs(-1)
    return res


def _assert_bit_identical(one, two):
    assert one.shape == two.shape
    a, b = torch.view_as_real(one), torch.view_as_real(two)
    assert bool(torch.isfinite(b).all())
    assert bool((two != SENTINEL).all()), "an output element was not written"
    assert float(two.abs().amax()) > 0
    assert torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} floats differ"


def test_pair_b64_1024_odd_rows_tail_stores_nothing():
    x, lam, sp = _white((1, 1, 7, 512), 31)
    (one, behind1), (two, behind2) = _both_forms(x, lam, sp, [0.02, 0.06], 3, 256, extra_rows=1)
    assert two.shape == (2, 1, 1, 7, 512)
    _assert_bit_identical(one, two)
    assert behind2.numel() == 512 and bool((behind2 == SENTINEL).all()), "the tail's second line stored a row"
    assert bool((behind1 == SENTINEL).all())


@pytest.mark.parametrize("Pw", [2048, 4096, 16384])
def test_pair_b64_planes_and_batches(Pw):
    x, lam, sp = _white((2, 1, 6, Pw // 2), 32 + Pw)
    (one, _), (two, _) = _both_forms(x, lam, sp, [0.03, 0.08], 3, Pw // 4)
    assert two.shape == (2, 2, 1, 6, Pw // 2)
    _assert_bit_identical(one, two)


def test_pair_b64_8192_mid_crop_is_the_default_path():
    from quantizationawarethzdoe_amd.propagation import asm_apply
    x, lam, sp = _white((1, 1, 4096, 4096), 33)
    zs = [0.02, 0.07]
    (one, _), (two, _) = _both_forms(x, lam, sp, zs, 2048, 2048)
    _assert_bit_identical(one, two)
    del one
    dflt = asm_apply(x, lam, sp, zs, 2048, 2048, True, 1)
    assert torch.equal(torch.view_as_real(dflt), torch.view_as_real(two))


def test_pair_b64_8192_other_crop():
    x, lam, sp = _white((1, 2, 6, 4000), 34, channels=2)
    (one, _), (two, _) = _both_forms(x, lam, sp, [0.03, 0.08], 3, 2096)
    assert two.shape == (2, 1, 2, 6, 4000)
    _assert_bit_identical(one, two)


def test_pair_b64_1024_against_the_table_algebra():
    """The pair form alone against complex128 algebra on its own exported table (9 rows: odd Hout)."""
    from quantizationawarethzdoe_amd import _lib
    a = tp._Asm(H=9, W=512, s=1, bl=None, z=0.05)
    assert a.Pw == 1024
    try:
        _lib.asm_row_pairs(1)
        out = a.prop(a.field).data.cpu()
    finally:
        _lib.asm_row_pairs(-1)
    Hc = a.table()
    ref = tr.asm_from_table(a.x, Hc, a.ph, a.pw, a.unpad)
    assert out.shape == ref.shape
    floor = tr.floor32(tr.asm_from_table, a.x, Hc, a.ph, a.pw, a.unpad, ref=ref)
    tp._judge("asm-rows-pair", "9x512 s1 Pw1024 none, pairs", out, ref, floor)
