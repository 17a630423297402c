"""The float64 restatement of the measurement kernels (tests/metrics_ref.py) pinned on closed forms, the grid
of spot_regions against qat.define_FoM, the library's exports and the host-side argument checks of
thz_metrics.hip -- all without a GPU."""
import ctypes
import math

import pytest
import torch

from quantizationawarethzdoe_amd import _lib, qat
from quantizationawarethzdoe_amd.utils import metrics
from tests import metrics_ref as mr

N_PIX, W0, C = 161, 12.0, (80.0, 80.0)  # a Gaussian I = exp(-2 r^2 / w^2), w = 12 pixels, on 161 x 161


def _gauss(n=N_PIX, w=W0, c=C):
    i = torch.arange(n, dtype=torch.float64)[:, None]
    j = torch.arange(n, dtype=torch.float64)[None, :]
    return torch.exp(-2 * ((i - c[0]) ** 2 + (j - c[1]) ** 2) / w ** 2)[None]


def test_power_in_a_circle_matches_the_closed_form():
    """sum of I over r <= a against (pi w^2 / 2)(1 - exp(-2 a^2 / w^2)): the quadrature error is the ring of
    pixels the circle cuts, each of unit area and of intensity at most exp(-2 (a - 1)^2 / w^2) ... computed
    here as the sum of I over the pixels whose centre lies within sqrt(1/2) of the circle."""
    I = _gauss()
    i = torch.arange(N_PIX, dtype=torch.float64)[:, None] - C[0]
    j = torch.arange(N_PIX, dtype=torch.float64)[None, :] - C[1]
    r = torch.sqrt(i * i + j * j)
    for a in (6.3, 12.4, 20.7):
        s = mr.region_sums(I, [("circ", C[0], C[1], a, 0.0)])[0, :, 0]
        closed = math.pi * W0 ** 2 / 2 * (1 - math.exp(-2 * a * a / W0 ** 2))
        ring = float(I[0][(r - a).abs() <= math.sqrt(0.5)].sum())
        assert abs(float(s[0]) - closed) <= ring, (a, float(s[0]), closed, ring)
        assert abs(float(s[0]) - closed) <= 0.05 * closed  # and resolved: the ring is a small part
        # the fraction of the total, as diffraction_efficiency reports it
        frac = float(mr.efficiency(I, [("circ", C[0], C[1], a, 0.0)])[0, 0])
        assert abs(frac - (1 - math.exp(-2 * a * a / W0 ** 2))) <= ring / float(s[1]) + 1e-9


def test_d4sigma_centroid_and_fwhm_of_a_gaussian():
    I = _gauss(c=(70.0, 91.0))
    pitch = 0.5e-3
    d4 = mr.d4sigma(I, [], pitch)[0, -1]
    assert torch.allclose(d4, torch.full((2,), 2 * W0 * pitch, dtype=torch.float64), rtol=1e-9)  # tails beyond 5 w
    cen = mr.centroid(I, [], pitch)[0, -1]
    want = torch.tensor([70.0 - 80.0, 91.0 - 80.0], dtype=torch.float64) * pitch
    assert torch.allclose(cen, want, rtol=0, atol=1e-12)
    # linear interpolation of a Gaussian between samples: the chord lies below the curve by at most
    # h^2 max|I''| / 8 = (4 / w^2) / 8 per unit intensity, over a slope of ~ sqrt(2 ln 2) / w per pixel at half height
    f = mr.fwhm(I, pitch)[0]
    exact = W0 * math.sqrt(2 * math.log(2)) * pitch
    tol = 2 * (0.5 / W0 ** 2) / (math.sqrt(2 * math.log(2)) / W0 * 0.5) * pitch
    assert float((f - exact).abs().max()) <= tol, (f, exact, tol)


def test_line_widths_edges_and_nearest_crossings():
    v = torch.tensor([[0.0, 1.0, 4.0, 1.0, 0.0, 3.0, 0.0],      # two lobes: the crossings nearest the peak
                      [4.0, 3.0, 1.0, 0.0, 0.0, 0.0, 0.0],      # peak at index 0: no left crossing
                      [0.0, 0.0, 0.0, 0.0, 1.0, 3.0, 4.0],      # peak at the last index: no right crossing
                      [2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0]])     # constant: lowest argmax, no crossing
    out = mr.line_widths(v, 0.5)
    assert out[0].tolist() == [4.0, 2.0, 1 + 1 / 3, 3 - 1 / 3, (3 - 1 / 3) - (1 + 1 / 3)]
    assert out[1, :2].tolist() == [4.0, 0.0] and math.isnan(out[1, 2]) and out[1, 3] == 2 - 1 / 2 and math.isnan(out[1, 4])
    assert out[2, :2].tolist() == [4.0, 6.0] and out[2, 2] == 4 + 1 / 2 and math.isnan(out[2, 3])
    assert out[3, :2].tolist() == [2.0, 0.0] and bool(torch.isnan(out[3, 2:]).all())


def test_peaks_ties_and_empty_regions():
    I = torch.ones(2, 5, 7, dtype=torch.float64)
    regions = [("circ", 2.0, 3.0, 1.2, 0.0), ("rect", 4.0, 6.0, 0.5, 1.5), ("circ", 40.0, 40.0, 2.0, 0.0)]
    peak, arg, cnt = mr.region_peaks(I, regions)
    assert cnt[0].tolist() == [5, 2, 0, 35]
    assert arg[0].tolist() == [1 * 7 + 3, 4 * 7 + 5, -1, 0] and peak[1].tolist() == [1.0, 1.0, 0.0, 1.0]
    assert mr.margin(regions[:2], 5, 7) >= 1e-3


def test_spot_regions_follow_the_grid_of_define_fom():
    res, dxy = [100, 100], 1e-3
    pos = [(a * 1e-3, b * 1e-3) for a, b in qat.FOCI_MM]
    reg = metrics.spot_regions(res, dxy, pos, 3e-3)
    assert reg.shape == (9, 3) and reg.dtype == torch.float64
    for p, r in zip(pos, reg):
        target = qat.define_FoM(res, dxy, 2.998e8 / 300e9, 0.2, list(p), device=torch.device("cpu"))[0, 0]
        ri, rj = round(float(r[0])), round(float(r[1]))
        # the rounded centre is an argmax of the target: it attains the maximum.  A spot on an axis falls half-way
        # between pixels 49 and 50 (49.5), where two (on both axes, four) pixels tie and argmax names the first
        assert float(target[ri, rj]) == float(target.max()), (p, r)
        if float(r[0]) % 1 != 0.5 and float(r[1]) % 1 != 0.5:
            assert (ri, rj) == divmod(int(target.argmax()), target.shape[-1]), (p, r)
    assert float(reg[0, 2]) == pytest.approx(3e-3 / (0.1 / 99))
    with pytest.raises(ValueError, match="square"):
        metrics.spot_regions([100, 50], dxy, pos, 3e-3)


def test_exports_and_alias():
    for name in ("thz_region_stats_workspace_size", "thz_region_stats_forward", "thz_region_stats_backward",
                 "thz_line_widths"):
        assert name in _lib.EXPORTED and hasattr(_lib.lib(), name)
    assert _lib.lib().thz_abi_version() == 9
    import quantizationawarethzdoe_amd as pkg
    pkg.install_reference_aliases()
    import utils.metrics as aliased
    assert aliased is metrics
    for fn in ("spot_regions", "diffraction_efficiency", "spot_uniformity", "centroid", "d4sigma", "encircled_energy",
               "fwhm", "focal_sweep"):
        assert callable(getattr(metrics, fn))
    u = metrics.spot_uniformity(torch.tensor([[1.0, 3.0, 2.0]], dtype=torch.float64))
    assert u.tolist() == [0.5]


def _desc(K=1, N=1, H=8, W=8, dtype=_lib.METRICS_C64, table=None):
    table = table or (_lib.Region * 17)(*[_lib.Region(kind=0, cr=1, cc=1, a=1, b=0)] * 17)
    return _lib.RegionStatsDesc(N=N, H=H, W=W, dtype=dtype, K=K, regions=ctypes.addressof(table),
                                regions_on_device=0), table


def test_argument_errors_reach_no_launch():
    """THZ_E_ARG from the loaded library, no GPU: the checks come before any device call."""
    h, err = _lib.lib(), lambda: _lib.lib().thz_last_error()
    n = ctypes.c_size_t(0)
    p = ctypes.c_void_p(4096)  # never dereferenced
    d, keep = _desc(K=17)
    assert h.thz_region_stats_workspace_size(ctypes.byref(d), ctypes.byref(n)) == _lib.THZ_E_ARG and b"regions" in err()
    assert h.thz_region_stats_forward(ctypes.byref(d), p, p, p, 1 << 20, None) == _lib.THZ_E_ARG
    assert h.thz_region_stats_backward(ctypes.byref(d), p, p, p, None) == _lib.THZ_E_ARG
    for bad in (dict(N=-1), dict(H=-1), dict(W=-3)):
        d, keep = _desc(**bad)
        assert h.thz_region_stats_workspace_size(ctypes.byref(d), ctypes.byref(n)) == _lib.THZ_E_ARG and b"shape" in err()
        assert h.thz_region_stats_forward(ctypes.byref(d), p, p, p, 1 << 20, None) == _lib.THZ_E_ARG
    d, keep = _desc(dtype=7)
    assert h.thz_region_stats_workspace_size(ctypes.byref(d), ctypes.byref(n)) == _lib.THZ_E_ARG and b"dtype" in err()
    d, keep = _desc(table=(_lib.Region * 17)(*[_lib.Region(kind=5)] * 17))
    assert h.thz_region_stats_workspace_size(ctypes.byref(d), ctypes.byref(n)) == _lib.THZ_E_ARG and b"kind" in err()
    d, keep = _desc(K=16, N=3, H=130, W=1030)
    assert h.thz_region_stats_workspace_size(ctypes.byref(d), ctypes.byref(n)) == _lib.THZ_OK
    assert n.value == (3 * 5 * 5 * 17 * 64 + 255) // 256 * 256  # 5 x 5 tiles of 32 x 256 per plane
    assert h.thz_region_stats_forward(ctypes.byref(d), p, p, ctypes.c_void_p(4100), n.value, None) == _lib.THZ_E_ARG
    assert b"workspace misaligned" in err()
    assert h.thz_region_stats_forward(ctypes.byref(d), p, p, p, n.value - 256, None) == _lib.THZ_E_WORKSPACE
    for level in (0.0, 1.0, -0.5, 1.5, math.nan):
        assert h.thz_line_widths(p, _lib.METRICS_F32, 4, 16, level, p, None) == _lib.THZ_E_ARG and b"level" in err()
    assert h.thz_line_widths(p, _lib.METRICS_F32, -1, 16, 0.5, p, None) == _lib.THZ_E_ARG
    assert h.thz_line_widths(p, _lib.METRICS_F32, 4, 0, 0.5, p, None) == _lib.THZ_E_ARG
    assert h.thz_line_widths(p, _lib.METRICS_C64, 4, 16, 0.5, p, None) == _lib.THZ_E_ARG and b"dtype" in err()


def test_python_argument_errors_before_any_launch():
    from quantizationawarethzdoe_amd import optics
    dev = torch.device("cpu")
    with pytest.raises(ValueError, match="17 regions"):
        optics.metrics.region_table([[1, 1, 1]] * 17, "circ", "region_stats", dev)
    with pytest.raises(ValueError, match=r"\[K, 3\]"):
        optics.metrics.region_table([[1, 1]], "circ", "region_stats", dev)
    with pytest.raises(ValueError, match="kind"):
        optics.metrics.region_table([[1, 1, 1]], "disc", "region_stats", dev)
    with pytest.raises(ValueError, match="rectangle"):
        optics.metrics.region_table([[1, 1, 1]], "rect", "region_stats", dev)
    with pytest.raises(ValueError, match="finite"):
        optics.metrics.region_table([[1, 1, -1]], "circ", "region_stats", dev)
    K, host, devtab = optics.metrics.region_table([[1, 2, 3, 4], [5, 6, 7, 8]], ["circ", "rect"], "region_stats", dev)
    assert K == 2 and devtab is None and (host[1].kind, host[1].cr, host[1].b) == (1, 5.0, 8.0)
    assert optics.metrics.region_table([], "circ", "region_stats", dev)[0] == 0
    with pytest.raises(RuntimeError, match="ROCm device"):
        optics.region_stats(torch.zeros(4, 4), [[1, 1, 1]])
    with pytest.raises(RuntimeError, match="ROCm device"):
        optics.line_widths(torch.zeros(4, 4))
