"""The measurement kernels on the GPU (thz_metrics.hip through optics.region_stats / line_widths and
utils.metrics), held to tests/metrics_ref.py in float64 on the CPU (pinned by tests/test_metrics_cpu.py).

    count, peak, argmax     equal to the restatement
    the five sums           |kernel - fp64| <= count 2^-52 |fp64| (non-negative terms: this bounds any order of
                            summation); the region tables keep every membership 1e-3 pixel^2 from a rounding
    backward                |kernel - fp64 autograd| <= 4 max(e32, 2^-24 |value|) in the maximum norm, e32 the
                            error of the restatement run in float32 (the rule of tests/test_losses_gpu.py)
    line_widths             peak, argmax and the NaN pattern equal; a crossing within
                            4 2^-53 (|t| + |v0|) / |v1 - v0| + 2^-52 W of the restatement's, from its own operands

Every comparison prints its ratio err / bound; THZ_METRICS_PARITY_LOG=<file> writes the largest per quantity
(profiles/metrics_parity_ratios.txt is such a run on an MI355X).
"""
import functools
import math
import os

import pytest
import torch

from quantizationawarethzdoe_amd import optics, qat
from quantizationawarethzdoe_amd.utils import metrics
from tests import metrics_ref as mr

pytestmark = pytest.mark.gpu

RATIOS = {}
SHAPES = [(1, 1), (37, 53), (64, 256), (130, 1030)]
DTYPES = {"complex64": torch.complex64, "float32": torch.float32, "complex128": torch.complex128}
EPS = 2.0 ** -52


def _dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _ratio_log():
    yield
    path = os.environ.get("THZ_METRICS_PARITY_LOG")
    if path:
        with open(path, "w") as fh:
            fh.write("# largest err / bound per quantity; bounds: sums count 2^-52 |fp64|; backward 4 max(e32, 2^-24 "
                     "|value|), maximum norm; crossings 4 2^-53 (|t| + |v0|) / |v1 - v0| + 2^-52 W\n")
            for k in sorted(RATIOS):
                fh.write(f"{k:28s} {RATIOS[k][0]:.4f}   ({RATIOS[k][1]})\n")


def _note(what, case, ratio):
    print(f"{what:26s} {case:60s} err / bound = {ratio:.4f}")
    if what not in RATIOS or ratio > RATIOS[what][0]:
        RATIOS[what] = (ratio, case)


def _bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.is_complex():
        a, b = torch.view_as_real(a), torch.view_as_real(b)
    wide = torch.int64 if a.element_size() == 8 else torch.int32
    return bool((a.view(wide) == b.view(wide)).all())


def _place(t, offset=0):
    """A contiguous device copy whose pointer is 16-byte aligned (offset 0) or one element past."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=_dev())
    v = buf[offset:offset + t.numel()].view(t.shape)
    v.copy_(t)
    assert (v.data_ptr() % 16 == 0) == (offset == 0 or t.element_size() == 16)
    return v.detach()


# ---- inputs, region tables and their float64 results, each made once ------------------------------
@functools.lru_cache(maxsize=None)
def _input(H, W, N, dtype):
    g = torch.Generator().manual_seed(1000 * H + 10 * W + N)
    dt = DTYPES[dtype]
    real = torch.float64 if dt == torch.complex128 else torch.float32
    if dt.is_complex:
        return torch.complex(torch.randn(N, H, W, generator=g, dtype=real), torch.randn(N, H, W, generator=g, dtype=real))
    return torch.rand(N, H, W, generator=g, dtype=real) + 0.01


@functools.lru_cache(maxsize=None)
def _table(name, H, W):
    """Rows (kind, cr, cc, a, b), every membership at least 1e-3 pixel^2 from a rounding (checked)."""
    m = float(min(H, W))
    if name == "none":
        rows = []
    elif name == "one":
        rows = [("circ", 0.41 * H + 0.137, 0.52 * W + 0.291, 0.31 * m + 0.618, 0.0)]
    else:
        rows = [("circ", 0.31 * H + 0.137, 0.42 * W + 0.291, 0.23 * m + 0.618, 0.0),
                ("circ", 0.36 * H + 0.219, 0.47 * W + 0.113, 0.19 * m + 0.377, 0.0),        # overlaps the first
                ("circ", 0.2, W - 1.3, 0.3 * m + 1.234, 0.0),                               # clipped by the edge
                ("circ", -50.5, -60.25, 7.3, 0.0),                                          # wholly outside
                ("rect", 0.5 * H, 0.5 * W, H + 0.5, W + 0.5),                               # covers the plane
                ("rect", 0.6 * H + 0.3, 0.3 * W + 0.2, 0.2 * H + 0.41, 0.25 * W + 0.37),    # overlaps the circles
                ("rect", H - 0.7, 0.1, 2.45, 0.3 * W + 0.45),                               # clipped by the corner
                ("rect", H + 20.5, 3.25, 4.4, 2.3)]                                         # wholly outside
        for k in range(8):
            cr, cc = (k + 0.5) / 8 * H + 0.173, ((3 * k) % 8 + 0.5) / 8 * W + 0.311
            rows.append(("circ", cr, cc, 1.618 + 0.35 * k, 0.0) if k % 2 == 0 else
                        ("rect", cr, cc, 1.37 + 0.4 * k, 2.21 + 0.3 * k))
    assert mr.margin(rows, H, W) >= 1e-3, (name, H, W, mr.margin(rows, H, W))
    return tuple(rows)


def _api(rows):
    """The table as optics.region_stats takes it."""
    return [list(r[1:]) for r in rows], [r[0] for r in rows]


@functools.lru_cache(maxsize=None)
def _ref(H, W, N, dtype, name):
    x, rows = _input(H, W, N, dtype), _table(name, H, W)
    return (mr.region_sums(x, rows),) + mr.region_peaks(x, rows)


def _check_stats(case, st, ref):
    sums, peak, arg, cnt = ref
    assert st.power.dtype == torch.float64 and st.argmax.dtype == torch.int64 and st.count.dtype == torch.int64
    assert torch.equal(st.count.cpu(), cnt), case
    assert torch.equal(st.argmax.cpu(), arg), case
    assert torch.equal(st.peak.cpu(), peak), case
    got = torch.cat((st.power[..., None], st.moment1, st.moment2), dim=-1).cpu()
    assert got.shape == sums.shape
    bound = cnt[..., None].double() * EPS * sums.abs()
    err = (got - sums).abs()
    assert bool((err <= bound).all()), (case, float((err - bound).max()))
    for q, what in enumerate(("S0", "Sr", "Sc", "Srr", "Scc")):
        ok = bound[..., q] > 0
        _note(f"region_stats {what}", case, float((err[..., q][ok] / bound[..., q][ok]).max()) if bool(ok.any()) else 0.0)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_region_stats_forward(shape, dtype):
    H, W = shape
    for N in (1, 3):
        xd = _place(_input(H, W, N, dtype))
        for name in ("none", "one", "sixteen"):
            regions, kinds = _api(_table(name, H, W))
            st = optics.region_stats(xd, regions, kinds)
            assert st.power.shape == (N, len(regions) + 1) and st.moment2.shape == (N, len(regions) + 1, 2)
            _check_stats(f"{dtype} {N}x{H}x{W} {name}", st, _ref(H, W, N, dtype, name))
            again = optics.region_stats(xd, regions, kinds)
            assert all(_bits(a, b) for a, b in zip(st, again)), "two calls differ"


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_region_stats_unaligned_view_and_device_table(dtype):
    """A pointer one element past 16-byte alignment takes the element-width loads; a region table given as a
    device tensor is read by the kernel.  Both give the aligned, host-table bits."""
    for H, W in ((37, 53), (130, 1030)):
        x = _input(H, W, 3, dtype)
        regions, kinds = _api(_table("sixteen", H, W))
        base = optics.region_stats(_place(x), regions, kinds)
        _check_stats(f"{dtype} 3x{H}x{W} unaligned", optics.region_stats(_place(x, 1), regions, kinds),
                     _ref(H, W, 3, dtype, "sixteen"))
        assert all(_bits(a, b) for a, b in zip(base, optics.region_stats(_place(x, 1), regions, kinds)))
        on_dev = torch.tensor(regions, dtype=torch.float64, device=_dev())
        assert all(_bits(a, b) for a, b in zip(base, optics.region_stats(_place(x), on_dev, kinds)))
        lead = optics.region_stats(_place(x).reshape(3, 1, H, W), regions, kinds)
        assert lead.power.shape == (3, 1, 17) and lead.moment1.shape == (3, 1, 17, 2)


def test_constant_plane_ties_take_the_lowest_index():
    for H, W in ((37, 53), (130, 1030)):
        rows = _table("sixteen", H, W)
        regions, kinds = _api(rows)
        x = torch.full((2, H, W), 0.75, dtype=torch.float32)
        st = optics.region_stats(x.to(_dev()), regions, kinds)
        peak, arg, cnt = mr.region_peaks(x, rows)
        m = mr.masks(rows, H, W).reshape(len(rows) + 1, -1)
        first = torch.tensor([int(torch.nonzero(r)[0]) if bool(r.any()) else -1 for r in m])
        assert torch.equal(arg[0], first)
        assert torch.equal(st.argmax.cpu(), arg) and torch.equal(st.peak.cpu(), peak) and torch.equal(st.count.cpu(), cnt)


# ---- backward -----------------------------------------------------------------------------------
def _grad_check(what, case, got, g64, g32):
    got = got.detach().cpu()
    got = torch.view_as_real(got).double() if got.is_complex() else got.double()
    g64 = torch.view_as_real(g64) if g64.is_complex() else g64
    g32 = torch.view_as_real(g32).double() if g32.is_complex() else g32.double()
    assert got.shape == g64.shape and bool(torch.isfinite(got).all())
    err = float((got - g64).abs().max())
    e32 = float((g32 - g64).abs().max())
    bound = 4 * max(e32, 2.0 ** -24 * float(g64.abs().max()))
    _note(what, case, err / bound if bound else float(err > 0))
    assert err <= bound, (what, case, err, e32, bound)


def _ref_grads(x, loss_of):
    """float64 autograd of the restatement and the same sequence in float32."""
    wide = torch.complex128 if x.is_complex() else torch.float64
    narrow = torch.complex64 if x.is_complex() else torch.float32
    x64 = x.to(wide).requires_grad_(True)
    g64, = torch.autograd.grad(loss_of(x64, False), x64)
    x32 = x.to(narrow).requires_grad_(True)
    g32, = torch.autograd.grad(loss_of(x32, True), x32)
    return g64, g32


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("shape", [(1, 1), (37, 53), (130, 1030)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_region_stats_backward_random_cotangents(shape, dtype):
    H, W = shape
    N = 2
    x = _input(H, W, 3, dtype)[:N]
    for name, offset in (("one", 0), ("sixteen", 1)):
        rows = _table(name, H, W)
        regions, kinds = _api(rows)
        g = torch.Generator().manual_seed(H + W + len(rows))
        G = torch.randn(N, len(rows) + 1, 5, generator=g, dtype=torch.float64)
        xd = _place(x, offset).requires_grad_(True)
        st = optics.region_stats(xd, regions, kinds)
        assert st.power.requires_grad and not st.peak.requires_grad and not st.argmax.requires_grad
        Gd = G.to(_dev())
        loss = (st.power * Gd[..., 0]).sum() + (st.moment1 * Gd[..., 1:3]).sum() + (st.moment2 * Gd[..., 3:5]).sum()
        got, = torch.autograd.grad(loss, xd)
        assert got.dtype == x.dtype and got.shape == x.shape
        g64, g32 = _ref_grads(x, lambda t, fp32: (mr.region_sums(t, rows, fp32=fp32) * G.to(torch.float32 if fp32 else
                                                                                           torch.float64)).sum())
        _grad_check("region_stats backward", f"{dtype} {N}x{H}x{W} {name} offset {offset}", got, g64, g32)


@pytest.mark.parametrize("dtype", ["complex64", "float32"])
def test_backward_through_efficiency_and_d4sigma(dtype):
    H, W, N = 37, 53, 2
    x = _input(H, W, 3, dtype)[:N]
    rows = _table("one", H, W)
    regions, kinds = _api(rows)
    pitch = 0.5
    xd = _place(x).requires_grad_(True)
    loss = metrics.diffraction_efficiency(xd, regions, kind=kinds).sum() + metrics.d4sigma(xd, regions, pitch, kind=kinds).sum()
    got, = torch.autograd.grad(loss, xd)

    def ref_loss(t, fp32):
        s = mr.region_sums(t, rows, fp32=fp32)
        mean = s[..., 1:3] / s[..., 0:1]
        d4 = 4 * torch.sqrt(s[..., 3:5] / s[..., 0:1] - mean * mean) * pitch
        return (s[:, :-1, 0] / s[:, -1:, 0]).sum() + d4.sum()

    g64, g32 = _ref_grads(x, ref_loss)
    _grad_check("efficiency + d4sigma grad", f"{dtype} {N}x{H}x{W}", got, g64, g32)


# ---- line widths ---------------------------------------------------------------------------------
def _check_lines(case, v, level=0.5):
    ref, ops = mr.line_widths(v, level, detail=True)
    lw = optics.line_widths(v.to(_dev()), level)
    assert lw.argmax.dtype == torch.int64 and lw.peak.shape == v.shape[:-1]
    assert torch.equal(lw.peak.cpu(), ref[:, 0]) and torch.equal(lw.argmax.cpu().double(), ref[:, 1]), case
    W = v.shape[-1]
    for q, got in ((0, lw.left.cpu()), (1, lw.right.cpu())):
        want = ref[:, 2 + q]
        assert torch.equal(torch.isnan(got), torch.isnan(want)), case
        ok = ~torch.isnan(want)
        t, v0, v1 = ops[ok, q, 0], ops[ok, q, 1], ops[ok, q, 2]
        bound = 4 * 2.0 ** -53 * (t.abs() + v0.abs()) / (v1 - v0).abs() + EPS * W
        err = (got[ok] - want[ok]).abs()
        if bool(ok.any()):
            _note("line_widths crossing", case, float((err / bound).max()))
        assert bool((err <= bound).all()), (case, err, bound)
    width = lw.width.cpu()
    assert torch.equal(torch.isnan(width), torch.isnan(ref[:, 4]))
    assert torch.equal(width[~torch.isnan(width)], (lw.right - lw.left).cpu()[~torch.isnan(width)])
    return lw


def _gauss_lines(W, centres, w, dtype=torch.float32):
    j = torch.arange(W, dtype=torch.float64)[None, :]
    c = torch.tensor(centres, dtype=torch.float64)[:, None]
    return torch.exp(-2 * (j - c) ** 2 / w ** 2).to(dtype)


def test_line_widths_gaussians_and_edges():
    v = _gauss_lines(97, [48.0, 20.3, 70.7, 0.0, 96.0, 3.2], 9.0)
    lw = _check_lines("gaussians W=97", v)
    assert math.isnan(float(lw.left[3])) and not math.isnan(float(lw.right[3]))   # peak at index 0
    assert math.isnan(float(lw.right[4])) and not math.isnan(float(lw.left[4]))   # peak at W - 1
    exact = 9.0 * math.sqrt(2 * math.log(2))
    # the chord between samples lies below the curve by at most max|I''| / 8 = (4 / w^2) / 8 = 0.006, over a slope of
    # 0.13 per sample at half height: 0.05 sample per side
    assert abs(float(lw.width[0]) - exact) < 0.1
    _check_lines("gaussians float64 level 0.135", v.double(), level=0.135)


def test_line_widths_takes_the_nearest_crossings():
    j = torch.arange(200, dtype=torch.float64)
    two = torch.exp(-2 * (j - 120) ** 2 / 64) + 0.8 * torch.exp(-2 * (j - 60) ** 2 / 64) + 0.7 * torch.exp(-2 * (j - 170) ** 2 / 36)
    lw = _check_lines("two lobes", two[None].float())
    assert 110 < float(lw.left[0]) < 120 < float(lw.right[0]) < 130  # not the outer lobes' flanks


@pytest.mark.parametrize("W", [1, 63, 64, 65, 1024, 1025, 3000])
def test_line_widths_lengths(W):
    g = torch.Generator().manual_seed(W)
    centres = [0.37 * W, 0.5 * W + 0.25, 0.0, W - 1.0, 0.81 * W]
    v = _gauss_lines(W, centres, max(W / 11.0, 0.8)) + 0.01 * torch.rand(len(centres), W, generator=g)
    _check_lines(f"W={W} float32", v)
    _check_lines(f"W={W} float64", v.double() * 3.7, level=0.3)
    flat = torch.full((2, W), 0.5)
    lw = optics.line_widths(flat.to(_dev()))
    assert lw.argmax.tolist() == [0, 0] and bool(torch.isnan(lw.width).all())


# ---- graph capture --------------------------------------------------------------------------------
def test_capture_and_replay_match_eager():
    H, W = 130, 1030
    rows = _table("sixteen", H, W)
    regions, kinds = _api(rows)
    g = torch.Generator().manual_seed(5)
    inputs = [_input(H, W, 3, "complex64"), torch.complex(torch.randn(3, H, W, generator=g), torch.randn(3, H, W, generator=g))]
    lines = [_gauss_lines(3000, [700.0, 12.5, 2999.0], 40.0), _gauss_lines(3000, [1500.2, 0.0, 80.0], 25.0)]
    G = torch.randn(3, 17, 5, generator=g, dtype=torch.float64).to(_dev())
    sx = inputs[0].to(_dev()).requires_grad_(True)
    sl = lines[0].to(_dev())

    def step(x, v):
        st = optics.region_stats(x, regions, kinds)
        loss = (st.power * G[..., 0]).sum() + (st.moment1 * G[..., 1:3]).sum() + (st.moment2 * G[..., 3:5]).sum()
        return tuple(st) + torch.autograd.grad(loss, x) + tuple(optics.line_widths(v))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(sx, sl)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(sx, sl)
    for x, v in zip(reversed(inputs), reversed(lines)):
        with torch.no_grad():
            sx.copy_(x)
            sl.copy_(v)
        graph.replay()
        torch.cuda.synchronize()
        eager = step(x.to(_dev()).requires_grad_(True), v.to(_dev()))
        for a, b in zip(out, eager):
            assert torch.equal(a.isnan(), b.isnan()) if a.is_floating_point() else True
            assert _bits(a, b)


# ---- end to end -----------------------------------------------------------------------------------
def test_four_focal_spots_efficiency_end_to_end():
    system = qat.FourFocalSpotsSystem(device=_dev())
    with torch.no_grad():
        field = system(0.5)
    assert tuple(field.data.shape) == (1, 1, 100, 100)
    pos = [(a * 1e-3, b * 1e-3) for a, b in qat.FOCI_MM]
    regions = metrics.spot_regions([100, 100], 1e-3, pos, 3.1e-3)
    rows = tuple(("circ", float(r[0]), float(r[1]), float(r[2]), 0.0) for r in regions)
    assert mr.margin(rows, 100, 100) >= 1e-3
    eff = metrics.diffraction_efficiency(field, regions)
    assert eff.shape == (1, 1, 9) and eff.dtype == torch.float64
    x = field.data.cpu().reshape(1, 100, 100)
    sums = mr.region_sums(x, rows)[0, :, 0]
    _, _, cnt = mr.region_peaks(x, rows)
    want = sums[:-1] / sums[-1]
    bound = (cnt[0, :-1].double() + cnt[0, -1].double() + 1) * EPS * want  # numerator, denominator, the division
    err = (eff.cpu().reshape(-1) - want).abs()
    _note("efficiency end to end", "FourFocalSpotsSystem 100x100, 9 spots", float((err / bound).max()))
    assert bool((err <= bound).all()), (err, bound)
    u = metrics.spot_uniformity(eff)
    assert u.shape == (1, 1) and 0.0 <= float(u) <= 1.0
    before = metrics.diffraction_efficiency(field, regions, reference=system.input_field)
    assert bool((before > 0).all()) and bool((before < 1).all())  # absorbing substrate: below the lossless ratio
    ee = metrics.encircled_energy(field, (49.5, 49.5), [2.3, 5.7, 11.1, 200.0])
    assert bool((ee[..., 1:] >= ee[..., :-1]).all()) and float(ee[0, 0, -1]) == 1.0


def test_focal_sweep_end_to_end():
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    from quantizationawarethzdoe_amd.Props.ASM_Prop import ASM_prop
    lam, dx, f = 2.998e8 / 300e9, 1e-3, 0.08
    x = optics.gaussian_beam(64, 64, dx, dx, [lam], [14e-3], [14e-3], device=_dev())
    x = optics.thin_lens(x.reshape(1, 1, 64, 64), dx, dx, f, [lam])
    field = ElectricField(x, wavelengths=lam, spacing=[dx, dx], device=_dev())
    prop = ASM_prop(z_distance=f, padding_scale=2, device=_dev())
    zs = [0.03 + 0.0065 * k + 0.0005 * (k % 3) for k in range(16)]  # not uniform, about the focus
    zx = prop.propagate_zx(field, zs, row=32)
    assert zx.shape == (16, 1, 1, 64)
    fs = metrics.focal_sweep(zx, zs, dx)
    peak, width, zl, zr, dof, lines, ops = mr.focal_sweep(zx.cpu().reshape(16, 1, 64), zs, dx, detail=True)
    assert torch.equal(fs.peak.cpu().reshape(16, 1), peak)
    got = (fs.width.cpu().reshape(16, 1) / dx)
    assert torch.equal(torch.isnan(got), torch.isnan(lines[..., 4]))
    ok = ~torch.isnan(got)
    bound = sum(4 * 2.0 ** -53 * (ops[..., q, 0].abs() + ops[..., q, 1].abs()) / (ops[..., q, 2] - ops[..., q, 1]).abs()
                + EPS * 64 for q in (0, 1))
    err = (got - lines[..., 4]).abs()
    _note("focal_sweep width", "64x64 lens-focused Gaussian, 16 planes", float((err[ok] / bound[ok]).max()))
    assert bool((err[ok] <= bound[ok]).all())
    for got_z, want_z in ((fs.z_left, zl), (fs.z_right, zr), (fs.depth_of_focus, dof)):
        # the same float64 interpolation of z_list from crossings that agree to the bound above
        assert torch.allclose(got_z.cpu().reshape(-1), want_z, rtol=1e-12, atol=0, equal_nan=True)
    print("depth of focus", float(fs.depth_of_focus), "m between", float(fs.z_left), float(fs.z_right))
    w = metrics.fwhm(field, dx)
    assert w.shape == (1, 1, 2) and torch.allclose(w.cpu().reshape(1, 2), mr.fwhm(x.cpu().reshape(1, 64, 64), dx), rtol=1e-12)
