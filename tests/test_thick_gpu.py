"""The thick-element DOE model on the GPU (optics.thick_doe, thz_thick_forward; csrc/thz_thick.hip).

Fused against the fp64 restatement tests/thick_ref.py on the table ASM_prop.create_kernel exports for
z = dz, so the rounding of the table's phase argument cancels.  Bound, on relative L2 and on max|err| /
rms: MARGIN = 4 times the error of the complex64 CPU run of the same algebra (thick_ref with
dtype=complex64: the kernels' fp32 op order for the screens, torch's fp32 CPU FFT for the steps) -- the
margin and the reasoning of tests/test_table_parity_gpu.py and DESIGN section 21: a different but equally
valid fp32 pipeline differs from that floor by small factors, never by an order of magnitude.  Every
case prints its line; THZ_THICK_PARITY_LOG=<file> appends them (profiles/thick_parity_ratios.txt).

Every height map carries the boundary values (0, below 0, every z_s, T, above T; thick_ref.
boundary_heights) in its first entries.  Pixels are one wavelength wide (1 mm at 300 GHz), eps = 2.66,
T = 4 mm: the regime the model is for.  A case's CPU results are formed once and shared.
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import table_ref as tr
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


def _judge(family, name, got, ref, floor):
    rel, mx = tr.errors(got, ref)
    line = (f"thick-parity {family:<14s} {name:<40s} floor32 {floor[0]:.3e} {floor[1]:.3e}  err {rel:.3e} {mx:.3e}"
            f"  ratio {rel / floor[0]:5.2f} {mx / floor[1]:5.2f}")
    print(line)
    log = os.environ.get("THZ_THICK_PARITY_LOG")
    if log:
        with open(log, "a") as f:
            f.write(line + "\n")
    assert rel <= MARGIN * floor[0] and mx <= MARGIN * floor[1], line


class _Case:
    """One geometry: the field and map on both sides, the exported table of one step, and -- formed once --
    the fp64 restatement and the floor of its complex64 run."""

    def __init__(self, shape, hw, S, convention="reference", bl="exact"):
        from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
        from quantizationawarethzdoe_amd.Props.ASM_Prop import ASM_prop
        B, C, H, W = shape
        self.S, self.convention, self.bl = S, convention, bl
        self.ph, self.pw = H // 2, W // 2
        self.x = _white(shape, 1000 * H + W + S)
        self.h = th.boundary_heights(hw[0], hw[1], T, S, seed=H + S)
        self.wl = [float(np.float32(C0 / (f * 1e9))) for f in GHZ[:C]]
        self.xd, self.hd = self.x.to(_dev()), self.h.to(_dev())
        field = ElectricField(self.xd, wavelengths=self.wl, spacing=[DX, DX], device=_dev())
        prop = ASM_prop(z_distance=th.step_size(T, S), padding_scale=1, bandlimit_kernel=bl is not None,
                        bandlimit_type=bl or "exact", device=_dev())
        prop.check_Zc = False
        self.Hc = prop.create_kernel(field).cpu()
        assert tuple(self.Hc.shape[-2:]) == (2 * H, 2 * W) and self.Hc.dtype == C64
        self.name = f"{B}x{C}x{H}x{W} map{hw[0]}x{hw[1]} S{S} {convention[:3]} bl={bl}"

    def run(self, method, **kw):
        from quantizationawarethzdoe_amd import optics
        return optics.thick_doe(self.xd, kw.pop("height", self.hd), self.wl, DX, EPS, TAND, T, self.S, padding_scale=1,
                                bandlimit=self.bl, convention=self.convention, method=method)

    def cpu(self, dtype):
        return th.thick_from_table(self.x, self.h, self.Hc, self.wl, EPS, TAND, T, self.S, self.ph, self.pw,
                                   sign=SIGN[self.convention], dtype=dtype)

    @functools.cached_property
    def ref(self):
        return self.cpu(tr.C128)

    @functools.cached_property
    def floor(self):
        return th.floor_of(self.cpu(C64), self.ref, self.S)


@functools.lru_cache(maxsize=None)
def _case(shape, hw, S, convention="reference", bl="exact"):
    return _Case(shape, hw, S, convention, bl)


SMALL = [((1, 1, 32, 32), (32, 32), 1, "reference", "exact"), ((1, 1, 32, 32), (32, 32), 1, "physical", "exact"),
         ((1, 1, 32, 32), (32, 32), 3, "reference", "exact"), ((1, 1, 32, 32), (32, 32), 3, "physical", "exact"),
         ((2, 3, 64, 32), (16, 8), 5, "reference", None), ((2, 3, 64, 32), (16, 8), 5, "reference", "exact")]
LARGE = ((1, 1, 1024, 1024), (1024, 1024), 4, "reference", "exact")
IDS = ["32-S1-ref", "32-S1-phy", "32-S3-ref", "32-S3-phy", "64x32-up-S5-nobl", "64x32-up-S5-exact", "1024-S4"]


@pytest.mark.parametrize("spec", SMALL + [LARGE], ids=IDS)
def test_fused_against_the_fp64_restatement(spec):
    c = _case(*spec)
    out, n = _launches(lambda: c.run("fused").cpu(), ("thick_rows", "thick_cols", "asm_tf_export", "asm_cols"))
    assert n == (c.S + 1, c.S, 1, 0), n   # two kernels per slab and the closing row pass, one table, no ASM pipeline
    assert out.shape == c.ref.shape and out.dtype == C64
    _judge("fused", c.name, out, c.ref, c.floor)


@pytest.mark.parametrize("spec", SMALL + [LARGE], ids=IDS)
def test_fused_against_compose(spec):
    c = _case(*spec)
    fused = c.run("fused").cpu()
    comp, n = _launches(lambda: c.run("compose").cpu(), ("thick_rows", "asm_cols"))
    assert n == (0, c.S), n
    _judge("fused/compose", c.name, fused, comp, c.floor)
    _judge("compose", c.name, comp, c.ref, c.floor)


def test_fused_against_compose_p4096():
    """[1, 1, 2048, 2048], S = 2, against compose only: the CPU restatement is too slow there.  The bound
    rests on the floor of the 1024^2, S = 4 case: the slabs' errors are independent and add in quadrature,
    so two slabs carry sqrt(2 / 4) of four slabs' floor; that the 4096-point transforms have one radix-2
    level more than the 2048-point ones (a factor of at most sqrt(12 / 11) on an FFT's error) is left out,
    which makes the bound tighter, not wider."""
    big = _case(*LARGE)
    floor = tuple(v * (2.0 / big.S) ** 0.5 for v in big.floor)
    c = _Case.__new__(_Case)
    c.S, c.convention, c.bl = 2, "reference", "exact"
    c.xd = _white((1, 1, 2048, 2048), 77).to(_dev())
    c.hd = th.boundary_heights(2048, 2048, T, 2, seed=78).to(_dev())
    c.wl = [float(np.float32(C0 / 300e9))]
    fused = c.run("fused")
    comp = c.run("compose")
    _judge("fused/compose", "1x1x2048x2048 S2 ref bl=exact", fused.cpu(), comp.cpu(), floor)


def test_thin_limit_is_the_fused_modulated_asm():
    """S = 1, sigma = -1: thz_asm_forward_modulated over T on the clipped map."""
    from quantizationawarethzdoe_amd import doe
    from quantizationawarethzdoe_amd import propagation as Pr
    c = _case(*SMALL[0])
    hc = c.hd.clamp(0.0, float(np.float32(T)))
    with torch.no_grad():
        pend = doe.PendingModulation(c.xd, hc, c.wl, EPS, TAND)
        thin = Pr.asm_propagate_modulated(pend, c.wl, (DX, DX), [th.step_size(T, 1)], c.ph, c.pw, True, 1)[0].cpu()
    _judge("thin-limit", c.name, c.run("fused").cpu(), thin, c.floor)


def test_graph_replay_is_bit_identical_to_the_eager_call():
    c = _case(*SMALL[2])
    eager = c.run("fused")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):   # one stream, no parallel branches
        captured = c.run("fused")
    captured.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager)


def test_auto_takes_compose_for_a_gradient_and_matches_autograd_of_the_restatement():
    """The derivative in h jumps where a pixel passes from one slab to the next (the slab's field changes), so
    the map here keeps the boundary values on which both roundings agree -- 0, below 0, above T -- and moves the
    entries that sit exactly on a z_s > 0 or on T half a slab down.  Tolerance: the 1e-4 relative L2 of the
    doe.modulate height-gradient tests (tests/test_doe_gpu.py)."""
    c = _case(*SMALL[2])
    dz = th.step_size(T, c.S)
    h = c.h.clone()
    flat = h.reshape(-1)
    flat[2] -= 0.5 * dz                  # T
    flat[5:4 + c.S] -= 0.5 * dz          # z_1 .. z_{S-1}
    G = _white(tuple(c.x.shape), 5)
    hd = h.to(_dev()).requires_grad_(True)
    out, n = _launches(lambda: c.run("auto", height=hd), ("thick_rows", "asm_cols"))
    assert n == (0, c.S), n
    (out * G.to(_dev()).conj()).real.sum().backward()
    h64 = h.clone().requires_grad_(True)
    ref = th.thick_from_table(c.x, h64, c.Hc, c.wl, EPS, TAND, T, c.S, c.ph, c.pw, sign=-1.0)
    (ref * G.to(tr.C128).conj()).real.sum().backward()
    got, want = hd.grad.cpu().double(), h64.grad
    rel = float((got - want).norm() / want.norm())
    print(f"thick-grad compose vs fp64 autograd rel-L2 {rel:.3e}")
    assert float(want.norm()) > 0 and rel <= 1e-4, rel
    with torch.no_grad():   # nothing requires grad: auto is fused
        _, n = _launches(lambda: c.run("auto"), ("thick_rows", "asm_cols"))
    assert n == (c.S + 1, 0), n
    with pytest.raises(RuntimeError, match="forward only"):
        c.run("fused", height=hd)


def test_element_and_ifta_result_equal_the_function():
    from quantizationawarethzdoe_amd import ifta
    from quantizationawarethzdoe_amd.Components.ThickDOE import ThickDOEElement
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    c = _case(*SMALL[5])
    want = c.run("fused")
    field = ElectricField(c.xd, wavelengths=c.wl, spacing=[DX, DX], device=_dev())
    el = ThickDOEElement(c.h, T, c.S, [EPS, TAND], padding_scale=1, device=_dev())
    out = el(field)
    assert isinstance(out, ElectricField) and torch.equal(out.data, want)
    res = ifta.IFTAResult(c.hd, None, None, (EPS, TAND), _dev())
    el2 = res.as_element(thick=dict(thickness=T, slices=c.S))
    assert isinstance(el2, ThickDOEElement) and torch.equal(el2(field).data, want)
    phys = ThickDOEElement(c.h, T, c.S, [EPS, TAND], convention="physical", device=_dev())(field).data
    assert not torch.equal(phys, want)
    with pytest.raises(TypeError, match="complex64"):
        el(ElectricField(c.xd.to(torch.complex128), wavelengths=c.wl, spacing=[DX, DX], device=_dev()))
