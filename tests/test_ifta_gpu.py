"""The IFTA projections and the designer on the GPU (thz_ifta.hip through optics.ifta_* and ifta.IFTA), held to
tests/ifta_ref.py in float64 on the CPU (pinned by tests/test_ifta_cpu.py).

    stats        each sum |kernel - fp64| <= count 2^-52 |fp64| (non-negative terms: this bounds any order of
                 summation); s and eff the float64 quotients of the kernel's own sums, bit for bit
    project      |kernel - fp64| <= 4 max(e32, 2^-24 |value|) in the maximum norm, e32 the error of the restatement
                 run in float32 (the rule of tests/test_losses_gpu.py); in place and out of place bit-equal
    doe project  q = 0: cyclic |h - fp64| <= 4 max(e32, 2^-24 h_max); q > 0: idx equal on every cell not set aside
                 (|g| < 1e-3 sum |terms|, or within the q = 0 bound of a midpoint between levels or of the q G
                 threshold; at most 1 % of a case), snapped cells lut[idx] and the others the q = 0 value bit for bit
    designer     three iterations at q = 0: heights (cyclic) and history rows within 4 max(e32, floor), floor =
                 2^-24 h_max / 2^-24 |value|; graph replay bit-equal to the eager loop; a 30-iteration run ends on
                 the table and its efficiency is within 4 |eff32 - eff64| of the restatement's

The 30-iteration run (seed 9, four evenly spaced levels): the restatement's float32 and float64 runs and the kernel
run make the same snap decision on every one of the 2500 cells, so the three maps are equal and |eff32 - eff64| is
the rounding of the final propagation and sums alone: the bound is meaningful as it stands.  The measured values
are in profiles/ifta_parity_ratios.txt.

Every comparison prints its ratio err / bound; THZ_IFTA_PARITY_LOG=<file> writes the largest per quantity
(profiles/ifta_parity_ratios.txt is such a run on an MI355X).
"""
import functools
import math
import os

import pytest
import torch

from quantizationawarethzdoe_amd import ifta, optics
from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
from quantizationawarethzdoe_amd.Props.ASM_Prop import ASM_prop
from quantizationawarethzdoe_amd.utils import metrics
from tests import ifta_ref as ir

pytestmark = pytest.mark.gpu

RATIOS, VALUES = {}, {}
SHAPES = [(1, 1), (37, 53), (64, 256), (130, 1030)]
LAM, EPS, TAND = 2.998e8 / 300e9, 2.66, 0.03
HM = ir.h_max(LAM, EPS)
U24, U52 = 2.0 ** -24, 2.0 ** -52
LUTS = {1: [0.3e-3], 2: [0.1e-3, 0.9e-3], 4: [0.05e-3, 0.2e-3, 0.9e-3, 1.5e-3], 10: [HM * i / 10 for i in range(10)]}


def _dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _ratio_log():
    yield
    path = os.environ.get("THZ_IFTA_PARITY_LOG")
    if path:
        with open(path, "w") as fh:
            fh.write("# largest err / bound per quantity; bounds: sums count 2^-52 |fp64|; project, heights, history "
                     "4 max(e32, 2^-24 |value|), maximum norm; set aside: share of cells, at most 0.01\n")
            for k in sorted(RATIOS):
                fh.write(f"{k:34s} {RATIOS[k][0]:.4f}   ({RATIOS[k][1]})\n")
            for k in sorted(VALUES):
                fh.write(f"{k:34s} {VALUES[k]}\n")


def _note(what, case, ratio):
    print(f"{what:30s} {case:56s} err / bound = {ratio:.4f}")
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
    assert (v.data_ptr() % 16 == 0) == (offset == 0)
    return v.detach()


# ---- inputs and their float64 results, each made once --------------------------------------------------
@functools.lru_cache(maxsize=None)
def _field(H, W, N, zeros=False):
    g = torch.Generator().manual_seed(1000 * H + 10 * W + N)
    U = torch.complex(torch.randn(N, H, W, generator=g), torch.randn(N, H, W, generator=g))
    if zeros:  # exact zeros of U, inside and outside the disc
        U = U.clone()
        U[0].reshape(-1)[::3] = 0
    return U


@functools.lru_cache(maxsize=None)
def _target(H, W, N, per_plane):
    g = torch.Generator().manual_seed(7 + 1000 * H + 10 * W + N)
    return torch.rand((N, H, W) if per_plane else (H, W), generator=g)


@functools.lru_cache(maxsize=None)
def _mask(H, W, kind):
    if kind == "none":
        return None
    if kind == "zero":
        return torch.zeros(H, W, dtype=torch.bool)
    i, j = torch.arange(H)[:, None], torch.arange(W)[None, :]
    return (i - 0.45 * H) ** 2 + (j - 0.55 * W) ** 2 <= (0.35 * max(min(H, W), 3)) ** 2


@functools.lru_cache(maxsize=None)
def _stats_ref(H, W, N, per_plane, mask):
    return ir.target_stats(_field(H, W, N).to(torch.complex128), _target(H, W, N, per_plane).double(), _mask(H, W, mask))


def _d(t):
    return None if t is None else t.to(_dev())


# ---- stats ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_stats(H, W, N):
    U = _field(H, W, N)
    for per_plane in (False, True):
        for mask in ("none", "disc", "zero"):
            for offset in ((0, 1) if mask == "disc" else (0,)):
                case = f"{N}x{H}x{W} T{'n' if per_plane else '1'} {mask} +{offset}"
                ref = _stats_ref(H, W, N, per_plane, mask)
                M = _mask(H, W, mask)
                got = optics.ifta_target_stats(_place(U, offset), _place(_target(H, W, N, per_plane), offset),
                                               None if M is None else _place(M, offset)).cpu()
                assert got.shape == (N, 6) and got.dtype == torch.float64 and not torch.isnan(got).any()
                n_in = H * W if M is None else int(M.sum())
                for k, count in ((0, H * W), (1, n_in), (2, n_in), (3, n_in)):
                    err, bound = (got[:, k] - ref[:, k]).abs(), count * U52 * ref[:, k].abs()
                    assert (err <= bound).all(), (case, optics.IFTA_STATS[k], err, bound)
                    live = bound > 0
                    if live.any():
                        _note(f"stats {optics.IFTA_STATS[k]}", case, float((err[live] / bound[live]).max()))
                s = torch.where(got[:, 3] == 0, torch.zeros(N, dtype=torch.float64), got[:, 2] / got[:, 3])
                eff = torch.where(got[:, 0] == 0, torch.zeros(N, dtype=torch.float64), got[:, 1] / got[:, 0])
                assert _bits(got[:, 4], s) and _bits(got[:, 5], eff), case
                if mask == "zero":
                    assert got[:, 1:].abs().max() == 0
    hist = torch.full((2, N, 6), -1.0, dtype=torch.float64, device=_dev())
    out = optics.ifta_target_stats(_d(U), _d(_target(H, W, N, False)), out=hist[1])
    assert out.data_ptr() == hist[1].data_ptr() and (hist[0] == -1).all()
    assert _bits(hist[1], optics.ifta_target_stats(_d(U), _d(_target(H, W, N, False))))


# ---- target project -------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_target_project(H, W, N):
    U = _field(H, W, N, zeros=True)
    for per_plane, mask in ((False, "disc"), (True, "none"), (True, "disc")):
        T, M = _target(H, W, N, per_plane), _mask(H, W, mask)
        s = ir.target_stats(U.to(torch.complex128), T.double(), M)[:, 4]
        for alpha in (1.0, 1.5):
            for beta in (0.0, 1.0):
                case = f"{N}x{H}x{W} T{'n' if per_plane else '1'} {mask} a{alpha} b{beta}"
                ref = ir.target_project(U.to(torch.complex128), T.double(), s, M, alpha, beta)
                r32 = ir.target_project(U, T, s.float(), M, alpha, beta)
                e32 = float((r32.to(torch.complex128) - ref).abs().max())
                bound = 4 * max(e32, U24 * float(ref.abs().max()))
                for offset in (0, 1):
                    Ud = _place(U, offset)
                    out = optics.ifta_target_project(Ud, _d(T), _d(s), _d(M), alpha, beta)
                    assert out.data_ptr() != Ud.data_ptr() and _bits(Ud, U)
                    err = float((out.cpu().to(torch.complex128) - ref).abs().max())
                    _note("project", case + f" +{offset}", err / bound if bound else 0.0)
                    assert err <= bound, (case, err, bound)
                    same = optics.ifta_target_project(Ud, _d(T), _d(s), _d(M), alpha, beta, out=Ud)
                    assert same.data_ptr() == Ud.data_ptr() and _bits(Ud, out), case
                # exact zeros inside the window take the amplitude itself, on the real axis
                inside = torch.ones(H, W, dtype=torch.bool) if M is None else M
                z = (U == 0) & inside
                if z.any():
                    want = torch.clamp(alpha * s.reshape(-1, 1, 1) * T.double().expand(N, H, W), min=0).float()
                    assert _bits(out.cpu()[z].real, want[z]) and (out.cpu()[z].imag == 0).all(), case


# ---- DOE project ----------------------------------------------------------------------------------------
DOE_CASES = [(1, 1, 1, 1), (5, 7, 1, 1), (5, 7, 3, 2), (16, 16, 8, 8), (50, 50, 2, 2)]


@functools.lru_cache(maxsize=None)
def _incident(H, W, N, kind):
    if kind == "none":
        return None
    g = torch.Generator().manual_seed(3 + 1000 * H + 10 * W + N)
    shape = (H, W) if kind == "one" else (N, H, W)
    return torch.complex(torch.randn(shape, generator=g), torch.randn(shape, generator=g))


def doe_case(hs, ws, rh, rw, N, akind, L, q):
    """The restatement's result in float64, the q = 0 bound and the cells set aside."""
    H, W = hs * rh, ws * rw
    U, A = _field(H, W, N), _incident(H, W, N, akind)
    ref = ir.doe_project(U.to(torch.complex128), None if A is None else A.to(torch.complex128), (hs, ws), LAM, EPS,
                         LUTS[L], q)
    r32 = ir.doe_project(U, A, (hs, ws), LAM, EPS, LUTS[L], 0.0)
    e32 = float(ir.cyclic(r32["hc"].double(), ref["hc"], HM).max())
    bound = 4 * max(e32, U24 * HM)
    aside = (ref["g"].abs() < 1e-3 * ref["terms"]) | (ir.decision_margin(ref, LUTS[L], HM, q) <= bound)
    return U, A, ref, bound, aside


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("hs,ws,rh,rw", DOE_CASES)
def test_doe_project(hs, ws, rh, rw, N):
    k = 0
    for akind in ("none", "one", "each"):
        for L in (1, 2, 4, 10):
            lut32 = torch.tensor(LUTS[L], dtype=torch.float32)
            h0 = None
            for q in (0.0, 0.5, 1.0):
                case = f"{N}x{hs}x{ws} r{rh}x{rw} A-{akind} L{L} q{q}"
                U, A, ref, bound, aside = doe_case(hs, ws, rh, rw, N, akind, L, q)
                k += 1
                qarg = torch.tensor([q], dtype=torch.float32, device=_dev()) if k % 2 else q  # tensor and number
                h, idx = optics.ifta_doe_project(_d(U), (hs, ws), LAM, EPS, LUTS[L], q=qarg, incident=_d(A))
                assert h.shape == (N, hs, ws) and h.dtype == torch.float32 and idx.dtype == torch.int32
                h, idx = h.cpu(), idx.cpu().long()
                if q == 0.0:
                    h0 = h
                    err = float(ir.cyclic(h.double(), ref["hc"], HM).max())
                    _note("doe height q=0", case, err / bound)
                    assert err <= bound, (case, err, bound)
                    on = idx >= 0  # only a cell exactly on a level snaps at q = 0
                    assert _bits(h[on], lut32[idx[on]])
                    continue
                share = float(aside.double().mean())
                _note("doe set aside / 0.01", case, share / 0.01)
                assert share <= 0.01, (case, share)
                keep = ~aside
                assert torch.equal(idx[keep], ref["idx"][keep]), (case, int((idx[keep] != ref["idx"][keep]).sum()))
                on = idx >= 0
                assert _bits(h[on], lut32[idx[on]]) and _bits(h[~on], h0[~on]), case
                if q == 1.0:
                    assert on.all()


def test_doe_project_wide_cells():
    """A cell wider than a workgroup's 256 lanes is summed in segments: r_w = 300, two cells, three rows."""
    g = torch.Generator().manual_seed(11)
    U = torch.complex(torch.randn(1, 3, 600, generator=g), torch.randn(1, 3, 600, generator=g))
    ref = ir.doe_project(U.to(torch.complex128), None, (1, 2), LAM, EPS, LUTS[4], 0.0)
    e32 = float(ir.cyclic(ir.doe_project(U, None, (1, 2), LAM, EPS, LUTS[4], 0.0)["hc"].double(), ref["hc"], HM).max())
    h, _ = optics.ifta_doe_project(_d(U), (1, 2), LAM, EPS, LUTS[4], q=0.0)
    err, bound = float(ir.cyclic(h.cpu().double(), ref["hc"], HM).max()), 4 * max(e32, U24 * HM)
    _note("doe height q=0", "1x1x2 r3x300", err / bound)
    assert err <= bound


# ---- the designer ---------------------------------------------------------------------------------------
FIELD, DOE = (100, 100), (50, 50)
LUT4 = [HM * i / 4 for i in range(4)]
REGIONS = metrics.spot_regions(FIELD, 1e-3, [(-20e-3, -20e-3), (20e-3, 20e-3), (-20e-3, 20e-3), (20e-3, -20e-3)], 4e-3)


@functools.lru_cache(maxsize=None)
def _spots():
    i, j = torch.arange(FIELD[0], dtype=torch.float64)[:, None], torch.arange(FIELD[1], dtype=torch.float64)[None, :]
    T = torch.zeros(FIELD, dtype=torch.float64)
    for cr, cc, a in REGIONS.tolist():
        T = torch.maximum(T, ((i - cr) ** 2 + (j - cc) ** 2 <= a * a).double())
    return T.float()


def _cfg(zs, scale):
    return dict(zs=list(zs), wavelength=LAM, spacing=1e-3, eps=EPS, tand=TAND, lut=LUT4, doe_shape=DOE,
                padding_scale=2, scale=scale, field_shape=FIELD)


def _designer(zs, scale):
    asm = ASM_prop(z_distance=zs[0], padding_scale=2, bandlimit_type="exact", device=_dev())
    asm.check_Zc = False
    return ifta.IFTA(asm, list(zs), LAM, 1e-3, EPS, TAND, LUT4, DOE, scale=scale)


def _init(seed):
    return torch.rand(DOE, generator=torch.Generator().manual_seed(seed)) * HM


@pytest.mark.parametrize("zs,scale", [((0.2,), "plane"), ((0.1, 0.15), "joint")])
def test_designer_trajectory(zs, scale):
    cfg, h0, T = _cfg(zs, scale), _init(5), _spots()
    h64, _, hist64 = ir.run(h0.double(), [0.0] * 3, T.double(), cfg, torch.complex128)
    h32, _, hist32 = ir.run(h0, [0.0] * 3, T, cfg, torch.complex64)
    res = _designer(zs, scale).run(_d(T), iters=3, q_schedule=[0.0] * 3, init=_d(h0), graph=False)
    case = f"Z{len(zs)} {scale}"
    e32 = float(ir.cyclic(h32.double(), h64, HM).max())
    err, bound = float(ir.cyclic(res.height.cpu().double(), h64, HM).max()), 4 * max(e32, U24 * HM)
    _note("designer height", case, err / bound)
    assert err <= bound, (case, err, bound)
    hist = res.history.cpu()
    assert hist.shape == (3, len(zs), 6)
    for k, name in enumerate(optics.IFTA_STATS):
        e32 = float((hist32[..., k].double() - hist64[..., k]).abs().max())
        err = float((hist[..., k] - hist64[..., k]).abs().max())
        bound = 4 * max(e32, U24 * float(hist64[..., k].abs().max()))
        _note(f"designer history {name}", case, err / bound)
        assert err <= bound, (case, name, err, bound)


def test_designer_graph_replay():
    T = _spots()
    des = _designer((0.1, 0.15), "plane")
    for seed in (5, 6):  # the second run replays the first one's graph
        h0 = _init(seed)
        a = des.run(_d(T), iters=6, init=_d(h0), graph=True)
        assert des.captures == 1
        b = des.run(_d(T), iters=6, init=_d(h0), graph=False)
        assert _bits(a.height, b.height) and _bits(a.idx, b.idx) and _bits(a.history, b.history), seed
        assert a.idx.dtype == torch.int64 and a.history.shape == (6, 2, 6)
    c = des.run(_d(T), iters=6, graph=True)  # the designer's own seeded draw
    assert des.captures == 1 and not _bits(c.height, a.height)


def _efficiency(height, zs):
    asm = ASM_prop(z_distance=zs[0], padding_scale=2, bandlimit_type="exact", device=_dev())
    asm.check_Zc = False
    res = ifta.IFTAResult(height, None, None, (EPS, TAND), _dev())
    field = ElectricField(torch.ones((1, 1) + FIELD, dtype=torch.complex64, device=_dev()), wavelengths=LAM,
                          spacing=1e-3, device=_dev())
    with torch.no_grad():
        return float(metrics.diffraction_efficiency(asm(res.as_element()(field)), REGIONS).sum())


def test_designer_full_run():
    """30 iterations of the default schedule; the module docstring says what |eff32 - eff64| measures here (all three
    runs end on the same map: kernel 0.722901, float64 0.722901, float32 0.722901, random init 0.023052)."""
    zs, T, h0 = (0.2,), _spots(), _init(9)
    cfg, qs = _cfg(zs, "plane"), ifta.default_q_schedule(30)
    res = _designer(zs, "plane").run(_d(T), iters=30, init=_d(h0), graph=True)
    idx, h = res.idx.cpu(), res.height.cpu()
    assert (idx >= 0).all() and _bits(h, torch.tensor(LUT4, dtype=torch.float32)[idx])
    h64, i64, _ = ir.run(h0.double(), qs, T.double(), cfg, torch.complex128)
    h32, i32, _ = ir.run(h0, qs, T, cfg, torch.complex64)
    e64 = float(ir.efficiency(h64, REGIONS.tolist(), cfg).sum())
    e32 = float(ir.efficiency(h32, REGIONS.tolist(), cfg, torch.complex64).sum())  # the whole restatement in float32
    got, start = _efficiency(res.height, zs), _efficiency(_d(h0), zs)
    VALUES["full run efficiency kernel"] = f"{got:.6f}"
    VALUES["full run efficiency fp64"] = f"{e64:.6f}"
    VALUES["full run efficiency fp32"] = f"{e32:.6f}"
    VALUES["full run efficiency random init"] = f"{start:.6f}"
    VALUES["full run cells differing"] = (f"kernel vs fp64 {int((idx != i64).sum())}, fp32 vs fp64 "
                                          f"{int((i32 != i64).sum())} of {idx.numel()}")
    print(VALUES)
    bound = 4 * abs(e32 - e64)
    _note("full run efficiency", "Z1 plane 30 it", abs(got - e64) / bound if bound else math.inf if got != e64 else 0.0)
    assert abs(got - e64) <= bound, (got, e64, e32)


def test_designer_errors():
    dev = _dev()
    asm = ASM_prop(z_distance=0.2, padding_scale=2, device=dev)
    mk = lambda **kw: ifta.IFTA(**{**dict(asm=asm, z_list=[0.2], wavelength=LAM, spacing=1e-3, eps=EPS, tand=TAND,
                                          lut=LUT4, doe_shape=DOE), **kw})
    T = _d(_spots())
    with pytest.raises(ValueError, match="B = C = 1"):
        mk(incident=torch.ones(2, 1, 100, 100, dtype=torch.complex64))
    with pytest.raises(ValueError, match="B = C = 1"):
        mk().run(T.expand(1, 2, 100, 100))
    with pytest.raises(TypeError, match="complex128"):
        mk(incident=torch.ones(100, 100, dtype=torch.complex128))
    with pytest.raises(TypeError, match="complex128"):
        optics.ifta_target_stats(torch.ones(4, 4, dtype=torch.complex128, device=dev), T[:4, :4])
    with pytest.raises(ValueError, match="whole number"):
        mk(doe_shape=(30, 50)).run(T)
    with pytest.raises(ValueError, match="whole number"):
        mk(doe_shape=(30, 50), incident=torch.ones(100, 100, dtype=torch.complex64))
    with pytest.raises(ValueError, match="do_unpad_after_pad"):
        mk(asm=ASM_prop(z_distance=0.2, padding_scale=2, do_unpad_after_pad=False, device=dev))
    with pytest.raises(ValueError, match="THZ_MAX_Z"):
        mk(z_list=[0.1 + 1e-4 * k for k in range(257)])
    with pytest.raises(ValueError, match="THZ_MAX_LUT"):
        mk(lut=[1e-5 * k for k in range(17)])
    with pytest.raises(TypeError, match="ASM_prop"):
        mk(asm=object())
    with pytest.raises(ValueError, match="scale"):
        mk(scale="each")
    with pytest.raises(ValueError, match="q_schedule"):
        mk().run(T, iters=3, q_schedule=[0.0, 1.0])
    # a table on the device must be read back, which a capture refuses (the rule of optics.lut_quantize)
    lut_dev = torch.tensor(LUT4, device=dev)
    U = torch.ones(1, 100, 100, dtype=torch.complex64, device=dev)
    optics.ifta_doe_project(U, DOE, LAM, EPS, lut_dev)  # outside a capture: read back
    q1 = torch.ones(1, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        with pytest.raises(RuntimeError, match="device tensor"):
            mk(lut=lut_dev)
        with pytest.raises(RuntimeError, match="device tensor"):
            optics.ifta_doe_project(U, DOE, LAM, EPS, lut_dev)
        h, idx = optics.ifta_doe_project(U, DOE, LAM, EPS, LUT4, q=q1)  # a host table is capturable
    g.replay()
    torch.cuda.synchronize()
    assert (idx.cpu() >= 0).all()
