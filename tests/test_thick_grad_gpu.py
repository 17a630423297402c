"""The native backward of the thick-element DOE on the GPU (optics.thick_doe(grad="fused"); thz_thick_forward_saved,
thz_thick_backward; csrc/thz_thick.hip).

Loss: L = Re<out, G> with a seeded white G.  Reference: fp64 autograd of the restatement tests/thick_ref.py on the
table ASM_prop.create_kernel exports for z = dz, so the rounding of the table's phase argument cancels.  Bound on
the relative L2 of grad_height and of grad_field: MARGIN = 4 times the error of the hand-written adjoint
restatement tests/thick_grad_ref.py run in complex64 on the CPU -- the floor convention of tests/test_thick_gpu.py
and tests/test_table_parity_gpu.py.  Every case prints its line (the compose path's ratio alongside, not gated);
THZ_THICK_GRAD_PARITY_LOG=<file> appends them (profiles/thick_grad_parity_ratios.txt).

Maps: thick_grad_ref.interior_heights -- thick_ref.boundary_heights with the entries on a face, on 0 or on T moved
half a slab inward (the derivative jumps there, and the kernels' strict rule and torch.clamp's inclusive one
differ only there); the entries below 0 and above T are kept.

Row-pass code paths (the host dispatch of thz_thick.hip): padded widths 64 .. 512 run the runtime-plan LDS path,
1024 and up the compile-time plans with the register hand-over.  The 32- and 64-wide cases and the xr = H + 1
case (Pw = 64) are on the first; [1, 1, 32, 512] (Pw = 1024, the smallest such) and the 1024^2 case on the second.
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import table_ref as tr
from tests import thick_grad_ref as tg
from tests import thick_ref as th

pytestmark = pytest.mark.gpu

MARGIN = 4.0
C0 = 2.998e8
DX = 1e-3
EPS, TAND = 2.66, 0.03
T = 4e-3
GHZ = (300, 280, 320)
C64 = torch.complex64
SIGN = {"reference": -1.0, "physical": 1.0}
ROWS, COLS, REDUCE = "thick_grad_rows", "thick_grad_cols", "thick_grad_reduce"


def _dev():
    return torch.device("cuda:0")


def _white(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, dtype=torch.complex128, generator=g).to(C64)


def _launches(fn, names):
    from quantizationawarethzdoe_amd import _lib
    _lib.timing_enable(True)
    try:
        _lib.timing_reset()
        out = fn()
        return out, tuple(_lib.timing_read(n)[1] for n in names)
    finally:
        _lib.timing_enable(False)


def _log(line):
    print(line)
    log = os.environ.get("THZ_THICK_GRAD_PARITY_LOG")
    if log:
        with open(log, "a") as f:
            f.write(line + "\n")


class _Case:
    """One geometry: field, map and G on both sides, the exported table of one step, and -- formed once -- the
    fp64 autograd gradients of the restatement and the floor of the complex64 adjoint restatement."""

    def __init__(self, shape, hw, S, convention="reference", bl="exact"):
        from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
        from quantizationawarethzdoe_amd.Props.ASM_Prop import ASM_prop
        B, C, H, W = shape
        self.S, self.convention, self.bl = S, convention, bl
        self.ph, self.pw = H // 2, W // 2
        self.x = _white(shape, 1000 * H + W + S)
        self.G = _white(shape, 7 + 1000 * W + H + S)
        self.h = tg.interior_heights(hw[0], hw[1], T, S, seed=H + S)
        self.wl = [float(np.float32(C0 / (f * 1e9))) for f in GHZ[:C]]
        self.xd, self.hd, self.Gd = self.x.to(_dev()), self.h.to(_dev()), self.G.to(_dev())
        field = ElectricField(self.xd, wavelengths=self.wl, spacing=[DX, DX], device=_dev())
        prop = ASM_prop(z_distance=th.step_size(T, S), padding_scale=1, bandlimit_kernel=bl is not None,
                        bandlimit_type=bl or "exact", device=_dev())
        prop.check_Zc = False
        self.Hc = prop.create_kernel(field).cpu()
        assert tuple(self.Hc.shape[-2:]) == (2 * H, 2 * W) and self.Hc.dtype == C64
        self.name = f"{B}x{C}x{H}x{W} map{hw[0]}x{hw[1]} S{S} {convention[:3]} bl={bl}"

    def args(self):
        return (self.wl, EPS, TAND, T, self.S, self.ph, self.pw, SIGN[self.convention])

    def run(self, method, x=None, h=None, grad="fused"):
        from quantizationawarethzdoe_amd import optics
        return optics.thick_doe(self.xd if x is None else x, self.hd if h is None else h, self.wl, DX, EPS, TAND, T,
                                self.S, padding_scale=1, bandlimit=self.bl, convention=self.convention, method=method,
                                grad=grad)

    def grads(self, method, grad="fused", want_x=True, want_h=True):
        """(out, grad_field, grad_height) of L = Re<out, G> on the GPU."""
        x = self.xd.clone().requires_grad_(want_x)
        h = self.hd.clone().requires_grad_(want_h)
        out = self.run(method, x, h, grad)
        (out * self.Gd.conj()).real.sum().backward()
        return out.detach(), x.grad, h.grad

    @functools.cached_property
    def ref(self):
        return tg.autograd_gradients(self.x, self.h, self.Hc, self.G, *self.args())

    @functools.cached_property
    def floor(self):
        """rel-L2 of the complex64 adjoint restatement against the fp64 reference: (grad_field, grad_height).
        Checked to be an fp32 pipeline's error over S slabs each way (thick_ref.floor_of's caps, twice)."""
        _, gx, gh = tg.gradients(self.x, self.h, self.Hc, self.G, *self.args(), dtype=C64)
        fx, fh = tg.rel_l2(gx, self.ref[1]), tg.rel_l2(gh, self.ref[2])
        for f in (fx, fh):
            assert 2.0 ** -24 <= f <= 8e-6 * self.S, f"floor32 {f:.3e} is not an fp32 pipeline's error"
        return fx, fh


@functools.lru_cache(maxsize=None)
def _case(shape, hw, S, convention="reference", bl="exact"):
    return _Case(shape, hw, S, convention, bl)


SMALL = [((1, 1, 32, 32), (32, 32), 1, "reference", "exact"), ((1, 1, 32, 32), (32, 32), 1, "physical", "exact"),
         ((1, 1, 32, 32), (32, 32), 3, "reference", "exact"), ((1, 1, 32, 32), (32, 32), 3, "physical", "exact"),
         ((2, 3, 64, 32), (16, 8), 5, "reference", None), ((2, 3, 64, 32), (16, 8), 5, "reference", "exact"),
         ((1, 1, 512, 32), (512, 32), 2, "reference", "exact"),    # xr = H + 1; columns on a compile-time plan
         ((1, 1, 32, 512), (32, 512), 2, "reference", "exact")]    # rows on a compile-time plan: the hand-over
IDS = ["32-S1-ref", "32-S1-phy", "32-S3-ref", "32-S3-phy", "64x32-up-S5-nobl", "64x32-up-S5-exact", "512x32-xr-S2",
       "32x512-handover-S2"]
UP_EXACT = SMALL[5]
LARGE = ((1, 1, 1024, 1024), (1024, 1024), 4, "reference", "exact")


@pytest.mark.parametrize("spec", SMALL, ids=IDS)
def test_gradients_against_fp64_autograd_of_the_restatement(spec):
    c = _case(*spec)
    (out, gx, gh), n = _launches(lambda: c.grads("fused"),
                                 ("thick_rows_saved", "thick_rows", "thick_cols", ROWS, COLS, REDUCE, "asm_cols"))
    # S + 1 row and S column launches each way, one reduction, no ASM pipeline
    assert n == (c.S, 1, c.S, c.S + 1, c.S, 1, 0), n
    assert torch.equal(out, c.run("fused", grad=None))
    _, cx, ch = c.grads("compose", grad=None)
    fx, fh = c.floor
    ex, eh = tg.rel_l2(gx.cpu(), c.ref[1]), tg.rel_l2(gh.cpu().double(), c.ref[2])
    kx, kh = tg.rel_l2(cx.cpu(), c.ref[1]), tg.rel_l2(ch.cpu().double(), c.ref[2])
    line = (f"thick-grad-parity {c.name:<40s} floor32 field {fx:.3e} height {fh:.3e}  err {ex:.3e} {eh:.3e}"
            f"  ratio {ex / fx:5.2f} {eh / fh:5.2f}  (compose ratio {kx / fx:5.2f} {kh / fh:5.2f})")
    _log(line)
    assert gx.dtype == C64 and gh.dtype == torch.float32 and gh.shape == c.h.shape
    assert ex <= MARGIN * fx and eh <= MARGIN * fh, line
    # below 0 and above T: exactly 0
    outside = (c.h <= 0) | (c.h >= float(np.float32(T)))
    assert bool(outside.reshape(-1)[1]) and bool(outside.reshape(-1)[3]) and torch.all(gh.cpu()[outside] == 0)


def test_large_case_against_compose():
    """[1, 1, 1024, 1024], S = 4, against compose's gradients: the fp64 autograd is too slow there.  Bound: 4 times
    the native-vs-compose relative L2 measured on the 64 x 32, S = 5 case, scaled by sqrt(4 / 5) (the slabs' errors
    add in quadrature, as in test_thick_gpu.test_fused_against_compose_p4096)."""
    s = _case(*UP_EXACT)
    _, sx, sh = s.grads("fused")
    _, kx, kh = s.grads("compose", grad=None)
    small = (tg.rel_l2(sx, kx), tg.rel_l2(sh, kh))
    c = _Case.__new__(_Case)
    c.S, c.convention, c.bl = LARGE[2], "reference", "exact"
    c.xd, c.Gd = _white(LARGE[0], 77).to(_dev()), _white(LARGE[0], 79).to(_dev())
    c.hd = tg.interior_heights(1024, 1024, T, c.S, seed=78).to(_dev())
    c.wl = [float(np.float32(C0 / 300e9))]
    out, gx, gh = c.grads("fused")
    assert torch.equal(out, c.run("fused", grad=None))
    _, cx, ch = c.grads("compose", grad=None)
    big = (tg.rel_l2(gx, cx), tg.rel_l2(gh, ch))
    scale = (c.S / s.S) ** 0.5
    line = (f"thick-grad-parity native/compose 1x1x1024x1024 S4: field {big[0]:.3e} height {big[1]:.3e}; 64x32 S5: "
            f"{small[0]:.3e} {small[1]:.3e}; ratio {big[0] / (small[0] * scale):5.2f} {big[1] / (small[1] * scale):5.2f}")
    _log(line)
    assert big[0] <= MARGIN * small[0] * scale and big[1] <= MARGIN * small[1] * scale, line


def test_backward_is_deterministic_and_graph_replay_is_bit_identical():
    c = _case(*UP_EXACT)
    out, gx, gh = c.grads("fused")
    out2, gx2, gh2 = c.grads("fused")
    assert torch.equal(gx, gx2) and torch.equal(gh, gh2) and torch.equal(out, out2)
    x = c.xd.clone().requires_grad_(True)
    h = c.hd.clone().requires_grad_(True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):   # one stream, no parallel branches
        o = c.run("fused", x, h)
        cgx, cgh = torch.autograd.grad((o * c.Gd.conj()).real.sum(), (x, h))
    for t in (o, cgx, cgh):
        t.detach().zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(o.detach(), out) and torch.equal(cgx, gx) and torch.equal(cgh, gh)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(cgx, gx) and torch.equal(cgh, gh)


def test_partial_requests():
    c = _case(*SMALL[2])
    names = ("thick_rows_saved", "thick_rows", "thick_cols", ROWS, COLS, REDUCE, "asm_cols")
    _, gx, gh = c.grads("fused")
    # field only: the plain forward (no stash), no reduction
    (_, fx, fh), n = _launches(lambda: c.grads("fused", want_h=False), names)
    assert n == (0, c.S + 1, c.S, c.S + 1, c.S, 0, 0), n
    assert fh is None and torch.equal(fx, gx)
    # height only: the saving forward, the reduction, no field store
    (_, hx, hh), n = _launches(lambda: c.grads("fused", want_x=False), names)
    assert n == (c.S, 1, c.S, c.S + 1, c.S, 1, 0), n
    assert hx is None and torch.equal(hh, gh)
    # "auto" with grad="fused" stays on the fused kernels on a native geometry
    (_, ax, ah), n = _launches(lambda: c.grads("auto"), names)
    assert n == (c.S, 1, c.S, c.S + 1, c.S, 1, 0) and torch.equal(ax, gx) and torch.equal(ah, gh)


def test_gradient_is_linear_in_the_field():
    """With the map fixed out = A x, so Re<x, grad_field> = Re<x, A^H G> = Re<A x, G> = L: the adjoint identity
    at the fp32 tolerance of tests/test_properties_gpu.py, 1e-5 ||A x|| ||G||."""
    for spec in (SMALL[5], SMALL[7]):
        c = _case(*spec)
        out, gx, _ = c.grads("fused", want_h=False)
        lhs = float((out.to(tr.C128) * c.Gd.to(tr.C128).conj()).real.sum())
        rhs = float((c.xd.to(tr.C128) * gx.to(tr.C128).conj()).real.sum())
        assert abs(lhs - rhs) <= 1e-5 * float(out.norm()) * float(c.Gd.norm()), (lhs, rhs)


def test_non_native_geometry_and_the_default_are_as_before():
    from quantizationawarethzdoe_amd import _lib, optics
    c = _case(*SMALL[2])
    hd = c.hd.clone().requires_grad_(True)
    # grad=None: auto takes compose for a gradient, fused refuses one
    out, n = _launches(lambda: c.run("auto", h=hd, grad=None), ("thick_rows", "asm_cols"))
    assert n == (0, c.S) and out.requires_grad
    with pytest.raises(RuntimeError, match="forward only"):
        c.run("fused", h=hd, grad=None)
    with torch.no_grad():
        _, n = _launches(lambda: c.run("auto", h=hd, grad=None), ("thick_rows", "asm_cols"))
    assert n == (c.S + 1, 0)
    with pytest.raises(ValueError, match="compose"):
        c.run("compose", h=hd)
    with pytest.raises(ValueError, match="grad must be"):
        c.run("auto", h=hd, grad="slice")
    # a 300-point padded plane: auto falls back to compose, fused raises the library's unsupported error
    x = _white((1, 1, 100, 100), 3).to(_dev())
    h = (torch.rand(100, 100, generator=torch.Generator().manual_seed(4)) * T).to(_dev()).requires_grad_(True)
    kw = dict(padding_scale=2, grad="fused")
    out, n = _launches(lambda: optics.thick_doe(x, h, c.wl, DX, EPS, TAND, T, 2, method="auto", **kw),
                       ("thick_rows", "asm_cols"))
    assert n == (0, 2) and out.requires_grad
    with pytest.raises(_lib.ThzError) as err:
        optics.thick_doe(x, h, c.wl, DX, EPS, TAND, T, 2, method="fused", **kw)
    assert err.value.code == _lib.THZ_E_UNSUPPORTED


def test_element_trains_a_parameter_map_on_the_native_backward():
    from quantizationawarethzdoe_amd import ifta
    from quantizationawarethzdoe_amd.Components.ThickDOE import ThickDOEElement
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    H = W = 64
    S = 4
    wl = [float(np.float32(C0 / 300e9))]
    x = torch.ones(1, 1, H, W, dtype=C64, device=_dev())
    field = ElectricField(x, wavelengths=wl, spacing=[DX, DX], device=_dev())
    h0 = (0.25 + 0.5 * torch.rand(H, W, generator=torch.Generator().manual_seed(9))) * T
    hmap = torch.nn.Parameter(h0.to(_dev()))
    el = ThickDOEElement(hmap, T, S, [EPS, TAND], padding_scale=1, device=_dev(), grad="fused")
    assert el.height_map is hmap
    spot = torch.zeros(H, W, dtype=torch.bool, device=_dev())
    spot[H // 2 - 4:H // 2 + 4, W // 2 - 4:W // 2 + 4] = True
    opt = torch.optim.Adam(el.parameters(), lr=2e-5)
    losses = []
    for _ in range(8):
        opt.zero_grad()
        out, n = _launches(lambda: el(field).data, ("thick_rows_saved", "asm_cols"))
        assert n == (S, 0), n
        inten = out.abs().pow(2)[0, 0]
        loss = -inten[spot].sum() / inten.sum()   # the share of the power in the focal spot
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("thick-grad training losses", " ".join(f"{v:.4f}" for v in losses))
    assert losses[-1] < losses[0], losses
    res = ifta.IFTAResult(hmap.detach(), None, None, (EPS, TAND), _dev())
    el2 = res.as_element(thick=dict(thickness=T, slices=S, grad="fused"))
    assert isinstance(el2, ThickDOEElement) and el2.grad == "fused"
