"""Every kernel family that can launch with more than 64 KiB of dynamic LDS has opted in.

A workgroup above 64 KiB of dynamic LDS launches only after its kernel's one-time opt-in
(csrc/thz_launch.hpp lds_opt_in; each unit lists its instantiations: czt_lds_attr and
czt_slice_lds_attr in csrc/thz_czt.hip, rsc_slice_lds_attr in csrc/thz_rsc.hip).  An instantiation
missing from its list launches below 64 KiB and fails above, so each case here is the smallest call
that puts one family above it: B = C = 1, Z <= 2, one entry point called once, THZ_OK (the glue
raises otherwise) and a finite result.  Values are checked by the families' own tests at small sizes.

Which launches cross 65536 B (csrc/thz_common.hpp, tw = 64 + n / 64 + 256 table entries):
* fft_lds_bytes_io(n), the compile-time powers of two, 8 (ceil((n + n / 16 + 1) / 2) + tw):
  38408 B at n = 8192, 74248 B at n = 16384 -- only the <16384> instantiations;
* fft_lds_bytes(n), the runtime plan, 8 (n + n / 16 + 1 + tw): 37896 B at 4096, 73224 B at 8192,
  108552 B at 12288, 143880 B at 16384 -- the <0> instantiations from n = 7300 or so.

CZT planes: a Bluestein length np2 = 16384 on one axis (m = 8200, M = 600: m + M - 1 = 8799 is no
power of two; M > 512 keeps the forward off the overlap-add form), the other axis 8 long, and the
reverse, forward and adjoint: czt_rows, czt_cols, czt_rows_adj, czt_cols_adj once each at <16384>.
CZT slice: czt_slice_line and czt_slice_line_adj at np2 = 16384 (W = 8200, outH = 64: 8263).
RSC slice: Pw = 8192 (below 64 KiB on every kernel) and Pw = 16384 (the runtime-plan accumulate at
143880 B beside compile-time rows and lines at 74248 B) are launched forward by
tests/test_rsc_zx_gpu.py (PLANS: 4 x 4096 and 4 x 8192) and backward by tests/test_rsc_zx_grad_gpu.py
(the same PLANS; WIDE is Pw = 16384), and are not repeated.  Not launched there: the runtime-plan
rows and lines above 64 KiB (Pw = 12288, no power of two) and VRS's Ez rows of the adjoint on the
runtime plan (Pw = 16384 with Ex, Ey planes, B = 2 as VRS requires).
The ASM planes at P = 8192 ... 16384 are tests/test_asm_gpu.py's (the fft_rows lengths, cfg2's
geometry, test_asm_largest_transform_p16384_properties) and the fp64 kernels' 139 KiB lines of
n = 8192 tests/test_f64_gpu.py's.
"""
import pytest
import torch

from quantizationawarethzdoe_amd import propagation as P

pytestmark = pytest.mark.gpu

LAM, SPACING, ZS = [1e-3], (0.25e-3, 0.25e-3), [0.05, 0.08]
LONG, SHORT, ZOOM, ZOOM_SLICE = 8200, 8, 600, 64


def _noise(*shape):
    g = torch.Generator().manual_seed(sum(shape))
    return torch.randn(*shape, dtype=torch.complex64, generator=g).to("cuda:0")


def _finite(t, shape):
    torch.cuda.synchronize()
    assert tuple(t.shape) == shape
    assert bool(torch.isfinite(torch.view_as_real(t)).all())


@pytest.mark.parametrize("H,W", [(SHORT, LONG), (LONG, SHORT)], ids=["rows16384", "cols16384"])
@pytest.mark.parametrize("adjoint", [False, True], ids=["forward", "adjoint"])
def test_czt_planes_np2_16384(H, W, adjoint):
    src = _noise(1, 1, ZOOM, ZOOM) if adjoint else _noise(1, 1, H, W)
    out = P.czt_apply(src, LAM, SPACING, ZS[0], ZOOM, ZOOM, 0.1e-3, 0.1e-3, adjoint=adjoint, field_hw=(H, W))
    _finite(out, (1, 1, H, W) if adjoint else (1, 1, ZOOM, ZOOM))


def test_czt_slice_np2_16384_forward():
    out = P.czt_slice_apply(_noise(1, 1, SHORT, LONG), LAM, SPACING, ZS, 3, ZOOM_SLICE, ZOOM_SLICE, 0.1e-3, 0.1e-3)
    _finite(out, (2, 1, 1, ZOOM_SLICE))


def test_czt_slice_np2_16384_adjoint():
    out = P.czt_slice_adjoint(_noise(2, 1, 1, ZOOM_SLICE), LAM, SPACING, ZS, 3, ZOOM_SLICE, ZOOM_SLICE, 0.1e-3,
                              0.1e-3, (SHORT, LONG))
    _finite(out, (1, 1, SHORT, LONG))


def test_rsc_slice_runtime_plan_12288_forward():
    out = P.rsc_slice_apply(_noise(1, 1, 4, 6144), LAM, SPACING, ZS, 1)
    _finite(out, (2, 1, 1, 6144))


def test_rsc_slice_runtime_plan_12288_adjoint():
    out = P.rsc_slice_adjoint(_noise(2, 1, 1, 6144), LAM, SPACING, ZS, 1, (1, 1, 4, 6144))
    _finite(out, (1, 1, 4, 6144))


def test_vrs_slice_16384_adjoint_ez_rows():
    out = P.rsc_slice_adjoint(_noise(2, 3, 1, 8192), LAM, SPACING, ZS, 1, (2, 1, 4, 8192), vectorial=True)
    _finite(out, (2, 1, 4, 8192))
