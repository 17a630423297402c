"""Property tests of the propagators on the GPU (SURVEY.md §4 layer 4), over hypothesis-drawn
shapes, paddings, distances, band limits, wavelengths and precisions -- size-independent facts
that hold for every input:

* linearity: A(a x + b y) = a A(x) + b A(y);
* adjoint identity: <A x, y> = <x, A^H y> through autograd (the backward kernels);
* contraction: ||A x|| <= ||x|| for ASM (zero-pad, unitary FFT, |H| <= 1 masks, crop) and the
  z-summed adjoint of a multi-plane forward equals the sum of the per-plane adjoints;
* agreement with the oracle on the drawn case (the fp64 restatement of the reference).

Tolerances: fp32 rel 1e-5 for the identities (one fp32 pipeline each way); vs the fp64 oracle
max(1e-4 (1 + k|z| / 1e3), 1.25 x the reference's own fp32 error on the drawn case); fp64 1e-12.
The fp32 CZT draws (both CZT tests) are value-checked twice: the whole call against the fp64 oracle
within the same max(1e-4 (1 + k|z| / 1e3), 1.25 x the reference's own fp32 error) -- the loose net --
and every (b, c) plane against the fp64 reference on the float32 grids within MARGIN x floor32 + PH on
relative L2 and max|err| / rms (tests/czt_ref.py, the bound of tests/test_czt_parity_gpu.py: about
1e-6 plus the fp32 rounding of the residual RS phase of the drawn geometry).
Examples are derandomized, but which ones run can still differ between runs (hypothesis'
generation depends on more than the seed), so every bound must hold for any draw.
"""
import os

import numpy as np
import pytest
import torch
from hypothesis import HealthCheck, assume, example, given, settings
from hypothesis import strategies as st

from oracle import thz_oracle as orc

pytestmark = pytest.mark.gpu
C0 = 2.998e8
# THZ_PROP_EXAMPLES=<n> THZ_PROP_RANDOM=1: a wider, randomly seeded sweep (run by hand to shake out
# bounds that only hold for the default draws)
SETTINGS = settings(max_examples=int(os.environ.get("THZ_PROP_EXAMPLES", "50")), deadline=None,
                    derandomize=os.environ.get("THZ_PROP_RANDOM", "0") != "1", database=None,
                    suppress_health_check=[HealthCheck.too_slow, HealthCheck.data_too_large])


def _dev():
    return torch.device("cuda:0")


def _rand(rng, shape, dtype):
    return torch.from_numpy(rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).to(dtype).to(_dev())


asm_cases = st.fixed_dictionaries({
    "B": st.integers(1, 2), "C": st.integers(1, 2), "H": st.integers(1, 160), "W": st.integers(1, 160),
    "s": st.sampled_from([1, 1.5, 2]), "z": st.floats(0.005, 0.4), "neg": st.booleans(),
    "bl": st.sampled_from(["exact", "approx", "none"]), "f": st.floats(200.0, 400.0),
    "dx": st.sampled_from([0.5, 1.0]), "f64": st.booleans(), "seed": st.integers(0, 2 ** 31 - 1),
})


@SETTINGS
@given(asm_cases)
def test_asm_properties(case):
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    from quantizationawarethzdoe_amd.Props.ASM_Prop import ASM_prop
    rng = np.random.default_rng(case["seed"])
    dt = torch.complex128 if case["f64"] else torch.complex64
    tol = 1e-12 if case["f64"] else 1e-5
    shape = (case["B"], case["C"], case["H"], case["W"])
    lam32 = torch.tensor([C0 / ((case["f"] + 37 * c) * 1e9) for c in range(case["C"])], dtype=torch.float32)
    wl = lam32.double() if case["f64"] else [float(v) for v in lam32]
    z = -case["z"] if case["neg"] else case["z"]
    prop = ASM_prop(z_distance=z, padding_scale=case["s"], bandlimit_kernel=case["bl"] != "none",
                    bandlimit_type="exact" if case["bl"] == "none" else case["bl"], device=_dev())

    def A(x):
        f = ElectricField(x, wavelengths=wl if case["C"] > 1 or case["f64"] else wl[0],
                          spacing=case["dx"] * 1e-3, device=_dev())
        return prop(f).data

    x, y = _rand(rng, shape, dt), _rand(rng, shape, dt)
    a, b = complex(rng.standard_normal(), rng.standard_normal()), complex(rng.standard_normal(), 0.5)
    Ax, Ay = A(x), A(y)
    lin = A(a * x + b * y)
    assert float((lin - (a * Ax + b * Ay)).norm() / (a * Ax + b * Ay).norm()) <= 10 * tol
    assert float(Ax.norm()) <= float(x.norm()) * (1 + 10 * tol)
    xg = x.clone().requires_grad_(True)
    out = A(xg)
    g = _rand(rng, tuple(out.shape), dt)
    gx, = torch.autograd.grad(out, xg, grad_outputs=g)
    lhs = torch.vdot(out.detach().reshape(-1).to(torch.complex128), g.reshape(-1).to(torch.complex128))
    rhs = torch.vdot(x.reshape(-1).to(torch.complex128), gx.reshape(-1).to(torch.complex128))
    assert abs(complex(lhs - rhs)) <= 10 * tol * abs(complex(lhs)) + 1e-30
    sp32 = torch.tensor([case["dx"] * 1e-3] * 2, dtype=torch.float32)
    kw = dict(bandlimit=case["bl"] != "none", bandlimit_type="exact" if case["bl"] == "none" else case["bl"])
    ref = orc.asm_forward(x.cpu().to(torch.complex128), lam32.double(), sp32.double(), z, case["s"], **kw)
    if case["f64"]:
        floor = 1e-11
    else:
        # the reference's own fp32 error on this case (the oracle in fp32 = the reference's fp32
        # arithmetic): near the evanescent cut-off of an unlimited band it reaches 2e-4 at k z ~ 1e3
        # rad, so the bound is the larger of the phase-scaled 1e-4 and 1.25 x that error (the rule
        # of tests/test_asm_gpu.py)
        ref32 = orc.asm_forward(x.cpu().to(torch.complex64), lam32, sp32, z, case["s"], **kw)
        e32 = float((ref32.to(torch.complex128) - ref).norm() / ref.norm())
        floor = max(1e-4 * (1 + abs(z) * 2 * np.pi / float(lam32.min()) / 1e3), 1.25 * e32)
    assert float((Ax.cpu().to(torch.complex128) - ref).norm() / ref.norm()) <= floor


@SETTINGS
@given(st.fixed_dictionaries({"H": st.integers(16, 120), "W": st.integers(16, 120), "Z": st.integers(2, 6),
                              "s": st.sampled_from([1, 2]), "seed": st.integers(0, 2 ** 31 - 1)}))
def test_asm_multi_plane_adjoint_is_the_sum_of_plane_adjoints(case):
    """One Z-summing adjoint launch == the sum over planes of single-plane adjoints (same kernels,
    different summation point: the spectrum vs the output), fp32 rel 1e-5."""
    from quantizationawarethzdoe_amd.propagation import asm_apply, asm_padding
    rng = np.random.default_rng(case["seed"])
    H, W, Z = case["H"], case["W"], case["Z"]
    ph, pw = asm_padding(H, W, (case["s"], case["s"]))
    zs = list(np.sort(rng.uniform(0.01, 0.3, Z)))
    lam = [float(np.float32(C0 / 300e9))]
    sp = [float(np.float32(1e-3))] * 2
    g = _rand(rng, (Z, 1, 1, H, W), torch.complex64)
    once = asm_apply(g, lam, sp, zs, ph, pw, True, 1, adjoint=True)
    summed = sum(asm_apply(g[k:k + 1], lam, sp, [z], ph, pw, True, 1, adjoint=True) for k, z in enumerate(zs))
    assert float((once - summed).norm() / summed.norm()) <= 1e-5


@SETTINGS
@given(st.fixed_dictionaries({"H": st.sampled_from([512, 1024, 2048]), "W": st.integers(100, 2048),
                              "Z": st.integers(1, 9), "uniform": st.booleans(), "B": st.integers(1, 2),
                              "dx": st.sampled_from([0.25, 0.5, 1.0]), "f": st.floats(220.0, 380.0),
                              "chunk": st.sampled_from([0, 2, 3]), "seed": st.integers(0, 2 ** 31 - 1)}))
def test_asm_pow2_columns_linearity_and_adjoint(case):
    """The power-of-two column kernels (P = 2H = 1024 .. 4096: compile-time radix-16 plans, the
    spectrum in registers across the planes, the plane recurrence on uniform sweeps) under drawn
    widths (row passes on the runtime plans where 2W is not a power of two), batches, spacings,
    plane lists (uniform or not) and z-chunks: the Z-plane forward is linear and its Z-summing
    adjoint launch is its adjoint, <A x, y> = <x, A^H y>, fp32 rel 1e-5."""
    from quantizationawarethzdoe_amd.propagation import asm_apply, asm_padding
    rng = np.random.default_rng(case["seed"])
    H, W, Z, B = case["H"], case["W"], case["Z"], case["B"]
    if case["uniform"]:
        zs = [float(v) for v in torch.linspace(0.02, 0.02 + 0.01 * (Z - 1), Z, dtype=torch.float32)]
    else:
        zs = [float(np.float32(v)) for v in rng.uniform(0.01, 0.3, Z)]
    ph, pw = asm_padding(H, W, (1, 1))
    lam = [float(np.float32(C0 / (case["f"] * 1e9)))]
    sp = [float(np.float32(case["dx"] * 1e-3))] * 2
    kw = dict(z_chunk=case["chunk"]) if case["chunk"] else {}
    x, y = _rand(rng, (B, 1, H, W), torch.complex64), _rand(rng, (B, 1, H, W), torch.complex64)
    a, b = complex(rng.standard_normal(), rng.standard_normal()), complex(rng.standard_normal(), 0.5)
    Ax = asm_apply(x, lam, sp, zs, ph, pw, True, 1, **kw)
    Ay = asm_apply(y, lam, sp, zs, ph, pw, True, 1, **kw)
    lin = asm_apply(a * x + b * y, lam, sp, zs, ph, pw, True, 1, **kw)
    ref = a * Ax + b * Ay
    assert float((lin - ref).norm() / ref.norm()) <= 1e-5
    g = _rand(rng, tuple(Ax.shape), torch.complex64)
    AHg = asm_apply(g, lam, sp, zs, ph, pw, True, 1, adjoint=True, **kw)
    lhs = torch.vdot(Ax.reshape(-1).to(torch.complex128), g.reshape(-1).to(torch.complex128))
    rhs = torch.vdot(x.reshape(-1).to(torch.complex128), AHg.reshape(-1).to(torch.complex128))
    assert abs(complex(lhs - rhs)) <= 1e-5 * float(Ax.norm()) * float(g.norm())


@SETTINGS
@given(st.fixed_dictionaries({"H": st.sampled_from([512, 1024]), "W": st.integers(200, 1024),
                              "Z": st.integers(3, 12), "dx": st.sampled_from([0.2, 0.25, 0.5, 1.0]),
                              "z0": st.floats(0.005, 0.2), "dz": st.floats(-0.02, 0.02),
                              "f": st.floats(250.0, 350.0), "seed": st.integers(0, 2 ** 31 - 1)}))
# found by a wide random sweep (k z = 1.9e3 rad at the last plane)
@example({"seed": 70, "H": 512, "W": 510, "Z": 11, "dx": 0.25, "z0": 0.125, "dz": 0.015625, "f": 334.0})
@example({"seed": 119, "H": 512, "W": 617, "Z": 11, "dx": 0.25, "z0": 0.09375, "dz": 0.015625, "f": 265.0})
def test_asm_uniform_sweep_matches_single_planes(case):
    """A uniform z-sweep on a power-of-two column length (padding scale 1: P = 1024 / 2048), where
    the column pass may advance the planes by the plane recurrence (csrc/thz_asm.hip
    recurrence_step_ok; taken per column when every step is an exact fp32 difference and the band
    stays under P/4), against each plane propagated on its own (one plane: the per-plane sincos):
    fp32 rel-L2 <= max(2e-5, ulp(k |z|) / 2) per plane; where |z| grows along the sweep the first
    plane is bit-identical (the recurrence starts there; a sweep towards the aperture runs its
    columns from the far end, so its bands still only narrow).  (2e-5 is
    tests/test_asm_recurrence_gpu.py's bound at cfg2's phases; the per-plane sincos form rounds its
    phase z sq <= k |z| to fp32 -- up to half an ulp per element, 3.6e-5 / 4.3e-5 rel-L2 at k z =
    1.9e3 / 1.3e3 rad (ulp 1.2e-4) in wide random sweeps -- while the recurrence carries the phase
    step in double.)"""
    from quantizationawarethzdoe_amd.propagation import asm_apply, asm_padding
    rng = np.random.default_rng(case["seed"])
    H, W, Z = case["H"], case["W"], case["Z"]
    zs = [float(v) for v in torch.linspace(case["z0"], case["z0"] + (Z - 1) * case["dz"], Z, dtype=torch.float32)]
    assume(min(abs(z) for z in zs) >= 1e-3)
    ph, pw = asm_padding(H, W, (1, 1))
    lam = [float(np.float32(C0 / (case["f"] * 1e9)))]
    sp = [float(np.float32(case["dx"] * 1e-3))] * 2
    x = _rand(rng, (1, 1, H, W), torch.complex64)
    multi = asm_apply(x, lam, sp, zs, ph, pw, True, 1)
    outward = all(abs(zs[k + 1]) >= abs(zs[k]) for k in range(Z - 1))
    for k, z in enumerate(zs):
        one = asm_apply(x, lam, sp, [z], ph, pw, True, 1)[0]
        if k == 0 and outward:
            assert torch.equal(multi[0], one)
        else:
            e = float((multi[k] - one).norm() / one.norm())
            kz = np.float32(2 * np.pi / lam[0] * abs(z))
            assert e <= max(2e-5, float(np.spacing(kz)) / 2), (k, z, e)


@SETTINGS
@given(st.fixed_dictionaries({"H": st.integers(1, 96), "W": st.integers(1, 96), "M": st.integers(1, 64),
                              "z": st.floats(0.1, 0.6), "f64": st.booleans(), "seed": st.integers(0, 2 ** 31 - 1)}))
def test_czt_linearity_and_adjoint(case):
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    from quantizationawarethzdoe_amd.Props.CZT_Prop import CZT_prop
    rng = np.random.default_rng(case["seed"])
    dt = torch.complex128 if case["f64"] else torch.complex64
    tol = 1e-12 if case["f64"] else 1e-5
    lam32 = torch.tensor([C0 / 300e9], dtype=torch.float32)
    wl = lam32.double() if case["f64"] else float(lam32[0])
    prop = CZT_prop(z_distance=case["z"], device=_dev())
    M = case["M"]

    def A(x):
        f = ElectricField(x, wavelengths=wl, spacing=[0.5e-3, 0.6e-3], device=_dev())
        return prop(f, M, M, 0.4e-3, 0.4e-3).data

    shape = (1, 1, case["H"], case["W"])
    x, y = _rand(rng, shape, dt), _rand(rng, shape, dt)
    p2 = [n & (n - 1) == 0 for n in (case["H"] + M - 1, case["W"] + M - 1)]
    if M == 1 and p2[1] and not p2[0]:
        # only the reference's second pass (m = W, M = 1) hits np2 == mp: it returns a [B, C, 1, 0]
        # field there (run here), and so does this build
        assert tuple(A(x).shape) == (1, 1, 1, 0)
        return
    if any(p2):
        # a power-of-two Bluestein length: the reference raises RuntimeError there (its slice keeps
        # M - 1 rows, or an MKL error at M = 1; Props/CZT_Prop.py:206,211), and so does this build
        with pytest.raises(RuntimeError, match="power of two"):
            A(x)
        return
    lin = A(2 * x - 1j * y)
    ref = 2 * A(x) - 1j * A(y)
    assert float((lin - ref).norm() / ref.norm()) <= 10 * tol
    xg = x.clone().requires_grad_(True)
    out = A(xg)
    g = _rand(rng, tuple(out.shape), dt)
    gx, = torch.autograd.grad(out, xg, grad_outputs=g)
    lhs = torch.vdot(out.detach().reshape(-1).to(torch.complex128), g.reshape(-1).to(torch.complex128))
    rhs = torch.vdot(x.reshape(-1).to(torch.complex128), gx.reshape(-1).to(torch.complex128))
    assert abs(complex(lhs - rhs)) <= 100 * tol * abs(complex(lhs))
    if not case["f64"]:
        _czt_values(A(x), x, [float(lam32[0])], (0.5e-3, 0.6e-3), case["z"], M, 0.4e-3)


def _czt_values(Ax, x, lam, sp, z, M, od):
    """A(x) of a drawn fp32 CZT case against the oracle in fp64 within max(1e-4 (1 + k|z| / 1e3), 1.25 x
    the reference's own fp32 error on the draw), and every (b, c) plane within MARGIN x floor32 + PH of the fp64
    reference on the float32 grids (tests/czt_ref.py; the bound of tests/test_czt_parity_gpu.py, its
    roundings count taken per pass from the form make_pass gives the drawn sizes)."""
    from tests import czt_ref as cr
    H, W = x.shape[-2:]
    xc = x.cpu()
    lam32 = torch.tensor(lam, dtype=torch.float32)
    sp32 = torch.tensor(sp, dtype=torch.float32)
    od32, z32 = cr.f32(od), cr.f32(z)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        ref = orc.czt_forward(xc.to(torch.complex128), lam32.double(), sp32.double(), z32, M, M, od32, od32)
    finally:
        torch.set_default_dtype(prev)
    e = float((Ax.detach().cpu().to(torch.complex128) - ref).norm() / ref.norm())
    floor = 1e-4 * (1 + abs(z32) * 2 * np.pi / float(lam32.min()) / 1e3)   # the phase-scaled rule of test_asm_properties
    if e > floor:  # only then does the reference's own fp32 error decide
        ref32 = orc.czt_forward(xc, lam32, sp32, torch.tensor(z32, dtype=torch.float32), M, M,
                                torch.tensor(od32, dtype=torch.float32), torch.tensor(od32, dtype=torch.float32))
        e32 = float((ref32.to(torch.complex128) - ref).norm() / ref.norm())
        assert e <= 1.25 * e32, (e, e32)
    geo = cr.Case(H, W, M, sp[0], sp[1], od, od, z, lam)
    ok, ratio, what = cr.plane_bounds_hold(geo, Ax.detach().cpu(), xc, (cr.pass_form(W, M), cr.pass_form(H, M)))
    assert ok, (ratio, what)


@SETTINGS
@given(st.fixed_dictionaries({"H": st.integers(520, 2100), "W": st.integers(520, 2100), "M": st.integers(1, 512),
                              "C": st.integers(1, 3), "z": st.floats(0.1, 0.6), "odx": st.sampled_from([0.2, 0.35, 0.5]),
                              "seed": st.integers(0, 2 ** 31 - 1)}))
def test_czt_overlap_add_linearity_and_adjoint(case):
    """cfg3-sized CZT geometries (the forward on the overlap-add kernels czt_rows_blk / czt_cols_blk
    wherever their 512-input blocks pay, partial last blocks and outputs not filling a 16-column V
    block included; the adjoint on the np2 kernels): linear, and the autograd backward its adjoint,
    |<A x, g> - <x, A^H g>| <= 1e-5 max(||A x|| ||g||, ||x|| ||A^H g||) (fp32: a 1 x 1 output sums
    ~5e5 random-phase terms to ~1e-3 of their magnitude, so each side's accumulation error is
    relative to the larger product)."""
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    from quantizationawarethzdoe_amd.Props.CZT_Prop import CZT_prop
    rng = np.random.default_rng(case["seed"])
    H, W, M, C = case["H"], case["W"], case["M"], case["C"]
    assume(all((n & (n - 1)) != 0 for n in (H + M - 1, W + M - 1)))  # power-of-two Bluestein: raises
    lam = [float(np.float32(C0 / ((240 + 40 * c) * 1e9))) for c in range(C)]
    prop = CZT_prop(z_distance=case["z"], device=_dev())
    od = case["odx"] * 1e-3

    def A(x):
        f = ElectricField(x, wavelengths=lam if C > 1 else lam[0], spacing=[0.5e-3, 0.5e-3], device=_dev())
        return prop(f, M, M, od, od).data

    B = 2 if 2 * C * H * W <= 3 * 2100 * 2100 else 1  # two batch planes while the call stays within 1 x 3 x 2100^2
    x, y = _rand(rng, (B, C, H, W), torch.complex64), _rand(rng, (B, C, H, W), torch.complex64)
    lin = A(2 * x - 1j * y)
    ref = 2 * A(x) - 1j * A(y)
    assert float((lin - ref).norm() / ref.norm()) <= 1e-5
    xg = x.clone().requires_grad_(True)
    out = A(xg)
    g = _rand(rng, tuple(out.shape), torch.complex64)
    gx, = torch.autograd.grad(out, xg, grad_outputs=g)
    lhs = torch.vdot(out.detach().reshape(-1).to(torch.complex128), g.reshape(-1).to(torch.complex128))
    rhs = torch.vdot(x.reshape(-1).to(torch.complex128), gx.reshape(-1).to(torch.complex128))
    scale = max(float(out.detach().norm()) * float(g.norm()), float(x.norm()) * float(gx.norm()))
    assert abs(complex(lhs - rhs)) <= 1e-5 * scale, (abs(complex(lhs - rhs)), scale)
    _czt_values(out, x, lam, (0.5e-3, 0.5e-3), case["z"], M, od)


@SETTINGS
@given(st.fixed_dictionaries({"H": st.integers(1, 96), "W": st.integers(1, 96), "C": st.integers(1, 2),
                              "z": st.floats(0.05, 0.6), "f": st.floats(250.0, 400.0),
                              "dx": st.sampled_from([1.0, 1.2, 2.0]), "f64": st.booleans(),
                              "seed": st.integers(0, 2 ** 31 - 1)}))
def test_rsc_linearity_adjoint_and_oracle(case):
    """RSC_prop (spatial RS kernel on the 2N grid, Props/RSC_Prop.py:129-215): linearity, the
    adjoint identity through autograd, and agreement with the oracle in fp64 within max(5e-4,
    1.25 x the reference's own fp32 error on the drawn case).  lambda <= 1.2 mm < sqrt(2) dx keeps
    clear of the reference's min-z crash (:112-117)."""
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    from quantizationawarethzdoe_amd.Props.RSC_Prop import RSC_prop
    rng = np.random.default_rng(case["seed"])
    dt = torch.complex128 if case["f64"] else torch.complex64
    tol = 1e-12 if case["f64"] else 1e-5
    C, H, W = case["C"], case["H"], case["W"]
    lam32 = torch.tensor([C0 / ((case["f"] + 23 * c) * 1e9) for c in range(C)], dtype=torch.float32)
    wl = lam32.double() if case["f64"] else ([float(v) for v in lam32] if C > 1 else float(lam32[0]))
    sp32 = torch.tensor([case["dx"] * 1e-3, case["dx"] * 1.1e-3], dtype=torch.float32)
    prop = RSC_prop(z_distance=case["z"], device=_dev())

    def A(x):
        f = ElectricField(x, wavelengths=wl, spacing=[float(v) for v in sp32], device=_dev())
        return prop(f).data

    x, y = _rand(rng, (1, C, H, W), dt), _rand(rng, (1, C, H, W), dt)
    Ax, Ay = A(x), A(y)
    if min(H, W) == 1:
        # the reference's [..., H:, W:] window of a 1-pixel axis is empty (run here), and so is this
        assert tuple(Ax.shape) == (1, C, 2 * (H // 2), 2 * (W // 2)) and Ax.numel() == 0
        return
    lin = A(2 * x - 1j * y)
    assert float((lin - (2 * Ax - 1j * Ay)).norm() / (2 * Ax - 1j * Ay).norm()) <= 10 * tol
    xg = x.clone().requires_grad_(True)
    out = A(xg)
    g = _rand(rng, tuple(out.shape), dt)
    gx, = torch.autograd.grad(out, xg, grad_outputs=g)
    lhs = torch.vdot(out.detach().reshape(-1).to(torch.complex128), g.reshape(-1).to(torch.complex128))
    rhs = torch.vdot(x.reshape(-1).to(torch.complex128), gx.reshape(-1).to(torch.complex128))
    assert abs(complex(lhs - rhs)) <= 100 * tol * abs(complex(lhs))
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        ref = orc.rsc_forward(x.cpu().to(torch.complex128), lam32.double(), sp32.double(), case["z"])
    finally:
        torch.set_default_dtype(prev)
    e = float((Ax.cpu().to(torch.complex128) - ref).norm() / ref.norm())
    if case["f64"]:
        assert e <= 1e-10
    else:
        ref32 = orc.rsc_forward(x.cpu(), lam32, sp32, torch.tensor(case["z"], dtype=torch.float32))
        e32 = float((ref32.to(torch.complex128) - ref).norm() / ref.norm())
        assert e <= max(5e-4, 1.25 * e32), (e, e32)


@SETTINGS
@given(st.fixed_dictionaries({"hs": st.integers(1, 80), "ws": st.integers(1, 80), "up": st.integers(1, 3),
                              "B": st.integers(1, 40), "C": st.integers(1, 4), "tol": st.sampled_from([0.0, 1e-5]),
                              "seed": st.integers(0, 2 ** 31 - 1)}))
def test_doe_modulate_vs_oracle(case):
    """DOE modulate forward and both gradients (Components/QuantizedDOE.py:47-126: noise, nearest
    upsampling of the height map to the field, transmission, product) vs the fp64 oracle's autograd
    over drawn map / field sizes (up to 3x nearest upsampling, odd sizes), batch sizes 1..40 (every
    batch-lane count of the backward's reduction) and 1..4 wavelengths: forward and field gradient
    rel 4e-6 (a few fp32 ulps of the largest phase, k (h + b)(sqrt(eps) - 1) <= 13 rad here: a
    single-element field has no averaging, 2.1e-6 was drawn); the height gradient per map element
    within 1e-5 of the sum of its terms' magnitudes (its B C terms, each the real part of a complex
    product, cancel: 2e-4 relative to the sum itself was drawn at a 1 x 1 map, B = 36, C = 2, and
    1.4e-5 relative to |Re| of a single term)."""
    from quantizationawarethzdoe_amd import doe
    from tests.golden_io import wavelengths
    g = torch.Generator().manual_seed(case["seed"])
    hs, ws, B, C = case["hs"], case["ws"], case["B"], case["C"]
    H, W = hs * case["up"], ws * case["up"]
    h = torch.rand(hs, ws, generator=g) * 1e-3
    u = torch.rand(hs, ws, generator=g)
    x = torch.randn(B, C, H, W, dtype=torch.complex64, generator=g)
    go = torch.randn(B, C, H, W, dtype=torch.complex64, generator=g)
    lam = wavelengths([240 + 30 * c for c in range(C)])
    hd = h.to(_dev()).requires_grad_(True)
    xd = x.to(_dev()).requires_grad_(True)
    out, hfull = doe.modulate(xd, hd, [float(v) for v in lam], 2.66, 0.03, tolerance=case["tol"], noise=u.to(_dev()))
    gx, gh = torch.autograd.grad(out, (xd, hd), grad_outputs=go.to(_dev()))
    ho = h.double().requires_grad_(True)
    xo = x.to(torch.complex128).requires_grad_(True)
    ro = orc.doe_modulate(xo, ho, lam.double(), torch.tensor(2.66, dtype=torch.float64),
                          torch.tensor(0.03, dtype=torch.float64), tolerance=case["tol"], noise_u01=u.double())
    go64 = go.to(torch.complex128)
    rgx, rgh = torch.autograd.grad(ro, (xo, ho), grad_outputs=go64, retain_graph=True)
    # the height gradient is a sum over B C (and the upsampled pixels) of terms
    # Re(conj(g) out dlog t/dh) that cancel, each the real part of a complex product that cancels
    # too: bound its error by the sum of the products' magnitudes |g| |out| |dlog t/dh|, the
    # oracle's gradient for g' = |g| (out dlog t/dh) / |out dlog t/dh| (dlog t/dh per wavelength:
    # -k/2 tand sqrt(eps) - i k (sqrt(eps) - 1))
    k = (2 * np.pi / lam.double())[None, :, None, None]
    n = float(np.sqrt(2.66))
    dlog = -0.5 * k * 0.03 * n - 1j * k * (n - 1)
    od = ro.detach() * dlog
    habs, = torch.autograd.grad(ro, ho, grad_outputs=go64.abs() * od / od.abs().clamp_min(1e-300))

    def rel(a, b):
        b = b.detach().numpy()
        return float(np.linalg.norm(a.detach().cpu().numpy() - b) / max(np.linalg.norm(b), 1e-300))

    assert hfull.shape == (H, W)
    assert rel(out, ro) <= 4e-6
    assert rel(gx, rgx) <= 4e-6
    err = (gh.detach().cpu().double() - rgh).abs()
    assert bool((err <= 1e-5 * habs + 1e-30).all()), float((err / habs.clamp_min(1e-300)).max())


LAYER_CLASSES = ["FullPrecisionDOELayer", "STEQuantizedDOELayer", "PSQuantizedDOELayer", "NaiveGumbelQuantizedDOELayer",
                 "SoftGumbelQuantizedDOELayerv2", "SoftGumbelQuantizedDOELayerv3",
                 "RotationallySymmetricFullPrecisionDOELayer", "RotationallySymmetricSTEQuantizedDOELayer",
                 "RotationallySymmetricPSQuantizedQuantizedDOELayer", "RotationallySymmetricNaiveGumbelQuantizedDOELayer",
                 "RotationallySymmetricScoreGumbelSoftQuantizedDOELayer"]


@SETTINGS
@given(st.fixed_dictionaries({"cls": st.sampled_from(LAYER_CLASSES), "n": st.integers(2, 48), "unit": st.booleans(),
                              "L": st.integers(2, 8), "hmax": st.sampled_from([0.5e-3, 1e-3, 1.5e-3]),
                              "frac": st.floats(0.0, 0.99), "C": st.integers(1, 2), "wscale": st.sampled_from([0.3, 3.0]),
                              "seed": st.integers(0, 2 ** 31 - 1)}))
# found by a wide random sweep: a saturated two-level softmax, whose direct backward form cancelled
# to a 1.2 % gradient error (csrc/thz_doe.hip softmax_bwd_level)
@example({"cls": "SoftGumbelQuantizedDOELayerv2", "n": 2, "unit": False, "L": 2, "hmax": 0.001,
          "frac": 0.794921875, "C": 1, "wscale": 0.3, "seed": 1537})
@example({"cls": "SoftGumbelQuantizedDOELayerv2", "n": 2, "unit": False, "L": 2, "hmax": 0.0015,
          "frac": 0.875, "C": 1, "wscale": 0.3, "seed": 1})
def test_doe_layer_vs_oracle(case):
    """Every QAT layer class of Components/QuantizedDOE.py (FP, STE, PSQ, naive Gumbel, score-Gumbel
    v2 / v3 and the five rotationally symmetric ones) over drawn DOE sizes (odd ones included), a
    mirrored unit cell or not, 2..8 levels, height limits, schedule positions and weight scales, with
    the Gumbel and height-noise draws injected: the layer's height map vs the oracle's in fp32
    (QuantizedDOE.py:286-1623 restated, the reference's arithmetic) to 5e-6 -- a LUT pick may flip
    where two perturbed scores tie to fp32 rounding, at most one pixel, and then the gradient is not
    compared -- and the weight gradient of sum |out|^2 through the modulated field vs the oracle's
    fp64 autograd within max(2e-4, 3 x the reference's own fp32 error) rel-L2."""
    from quantizationawarethzdoe_amd.Components import QuantizedDOE as Q
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    from tests.golden_io import wavelengths
    cls, n, L = case["cls"], case["n"], case["L"]
    rot = cls.startswith("RotationallySymmetric")
    unit = case["unit"] and not rot and not cls.endswith("v2") and n % 2 == 0
    g = torch.Generator().manual_seed(case["seed"])
    psq = "PSQ" in cls
    optim = {"c_s": 100, "tau_max": 20 if psq else 2.5, "tau_min": 1 if psq else 1.5}
    doe_params = {"doe_size": [n, n], "doe_dxy": 1e-3, "doe_level": L, "num_unit": 2 if unit else None,
                  "height_constraint_max": case["hmax"], "tolerance": 1e-5, "material": [2.66, 0.03]}
    torch.manual_seed(case["seed"] % 1000)
    if cls.endswith("FullPrecisionDOELayer"):
        layer = getattr(Q, cls)(doe_params, device=_dev())
    else:
        layer = getattr(Q, cls)(doe_params, optim, device=_dev())
    param = next(iter(layer.parameters()))
    w0 = torch.randn(param.shape, generator=g) * case["wscale"]
    with torch.no_grad():
        param.copy_(w0)
    frac = None if cls.endswith(("FullPrecisionDOELayer", "STEQuantizedDOELayer")) else case["frac"]
    freqs = [300 + 20 * c for c in range(case["C"])]
    lam = wavelengths(freqs)
    x = torch.randn(1, case["C"], n, n, dtype=torch.complex64, generator=g)
    draws = {}

    def fake_noise(shape, like):
        draws["expo"] = torch.empty(tuple(shape)).exponential_(generator=g)
        return draws["expo"].to(like.device)

    def fake_rand(t, *a, **k):
        draws["unif"] = torch.rand(tuple(t.shape), generator=g)
        return draws["unif"].to(device=t.device, dtype=t.dtype)

    layer._gumbel_noise = fake_noise
    orig = torch.rand_like
    torch.rand_like = fake_rand
    try:
        field = ElectricField(x.to(_dev()), wavelengths=[float(v) for v in lam] if case["C"] > 1 else float(lam[0]),
                              spacing=[1e-3, 1e-3], device=_dev())
        out = layer(field, iter_frac=frac)
        (out.data.abs() ** 2).sum().backward()
    finally:
        torch.rand_like = orig
    lut = torch.linspace(0, torch.tensor(case["hmax"]), L + 1)[:-1]
    wo = w0.clone().requires_grad_(True)
    ho = orc.layer_height_map(cls, wo, lut, torch.tensor(case["hmax"]), lam.min(), 2.66, frac, optim,
                              2 if unit else None, [n, n], expo=draws.get("expo"))
    hn = layer.height_map.detach().cpu()
    assert tuple(hn.shape) == tuple(ho.shape) == (n, n)
    # 5e-6: the smooth maps (FP, PSQ's sum of L sigmoids, the v3 blend) carry a few fp32 ulps of
    # their own (the reference's fp32 is 8e-7 from fp64 on a drawn PSQ map); a LUT flip is a
    # whole level step, >= hmax / 8
    mism = int((~torch.isclose(hn, ho.detach(), rtol=5e-6, atol=1e-12)).sum())
    assert mism <= 1, mism
    if mism:
        return
    def oracle_grad(dt, wscale=1.0):
        """d sum |out|^2 / d weight: the layer in dt (float32 = the reference's arithmetic), the
        modulation in fp64; wscale perturbs the weights by a few ulps"""
        w = (w0.clone().to(dt) * wscale).requires_grad_(True)
        e = draws.get("expo")
        h = orc.layer_height_map(cls, w, lut.to(dt), torch.tensor(case["hmax"], dtype=dt), lam.min().to(dt), 2.66,
                                 frac, optim, 2 if unit else None, [n, n], expo=None if e is None else e.to(dt))
        r = orc.doe_modulate(x.to(torch.complex128), h.double(), lam.double(), torch.tensor(2.66, dtype=torch.float64),
                             torch.tensor(0.03, dtype=torch.float64), tolerance=1e-5, noise_u01=draws["unif"].double())
        (r.abs() ** 2).sum().backward()
        return w.grad.detach().double()

    gn, g64, g32 = param.grad.detach().cpu().double(), oracle_grad(torch.float64), oracle_grad(torch.float32)
    if float(g64.abs().max()) == 0:
        assert float(gn.abs().max()) == 0
    else:
        # a saturated Gumbel-softmax derivative p (1 - p) loses digits in fp32 (the reference's
        # autograd and this build's kernel alike, each its own way): bound by the reference's own
        # fp32 error on the drawn case -- 0.7 % was drawn at a 2 x 2 v2 map (this build 0.2 %), and
        # 4.3e-5 at a 37 x 37 rotationally symmetric v3 map (this build 1.04e-4, from elements 1e-3 of
        # the largest off by 5 %); a wrong formula is off by O(1) on the largest elements
        # and by the spread of the reference's fp32 arithmetic under a 2-ulp weight perturbation
        # (the conditioning of the drawn case: 0.6 % drawn at a saturated 2 x 2 rotationally
        # symmetric v3 map whose fp32 reference happened to land 0.06 % from fp64)
        e32 = float((g32 - g64).norm() / g64.norm())
        ep = max(float((oracle_grad(torch.float32, 1.0 + k * 2.0 ** -22) - g64).norm() / g64.norm()) for k in (1, -1))
        assert float((gn - g64).norm() / g64.norm()) <= max(2e-4, 3 * e32, 3 * ep), (e32, ep)


@SETTINGS
@given(st.fixed_dictionaries({"H": st.integers(2, 96), "W": st.integers(2, 96), "B": st.integers(1, 3),
                              "C": st.integers(1, 2), "dx": st.sampled_from([0.5e-3, 1e-3, 1.3e-3]),
                              "dy": st.sampled_from([0.5e-3, 1e-3, 0.7e-3]), "f": st.floats(0.05, 0.5),
                              "kind": st.sampled_from(["rect", "circ"]), "size": st.floats(2e-3, 0.12),
                              "Ho": st.integers(1, 96), "Wo": st.integers(1, 96),
                              "zoom": st.sampled_from([0.25, 0.5, 1.0, 1.7, 3.0]), "seed": st.integers(0, 2 ** 31 - 1)}))
# found by a wide random sweep: the lens coefficient formed as a correctly rounded division gave
# 8.1e-6 against the reference's 3.4e-6 (torch forms pi / (lambda f) as reciprocal x pi)
@example({"H": 83, "W": 2, "B": 1, "C": 1, "dx": 0.0013, "dy": 0.0005, "f": 0.07876511813361319, "kind": "rect",
          "size": 0.0625, "Ho": 1, "Wo": 1, "zoom": 0.25, "seed": 0})
def test_optics_elements_vs_oracle(case):
    """Thin lens (Components/Thin_Lens.py:31-85), aperture masks (Components/Aperture.py:61-118) and
    the field resampler (Addons/Field_Resampler.py:56-118) over drawn shapes, spacings, focal
    lengths, aperture sizes and output grids: the lens within max(4e-6, 2 x the reference's fp32
    error) of the fp64 oracle (its phase pi r^2 / (lambda f) reaches ~10^3 rad here), the aperture
    bit-exact against the oracle's fp32 mask, the resampler and its gradient per element within the
    effect of a few ulps of its fp32 sampling coordinates (+ 1e-5 relative) of the oracle's fp64
    grid_sample."""
    from quantizationawarethzdoe_amd.Addons.Field_Resampler import Field_Resampler
    from quantizationawarethzdoe_amd.Components.Aperture import ApertureElement
    from quantizationawarethzdoe_amd.Components.Thin_Lens import Thin_LensElement
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    from tests.golden_io import wavelengths
    g = torch.Generator().manual_seed(case["seed"])
    B, C, H, W = case["B"], case["C"], case["H"], case["W"]
    lam = wavelengths([300 + 25 * c for c in range(C)])
    x = torch.randn(B, C, H, W, dtype=torch.complex64, generator=g)
    dx, dy = case["dx"], case["dy"]

    def ef(data):
        return ElectricField(data, wavelengths=[float(v) for v in lam] if C > 1 else float(lam[0]),
                             spacing=[dx, dy], device=_dev())

    def rel(a, b):
        a, b = a.detach().cpu().to(torch.complex128), b.detach().to(torch.complex128)
        return float((a - b).norm() / max(float(b.norm()), 1e-300))

    sp32 = torch.tensor([dx, dy], dtype=torch.float32)
    # thin lens
    lens = Thin_LensElement(case["f"])(ef(x.to(_dev()))).data
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        r64 = orc.thin_lens(x.to(torch.complex128), float(sp32[0]), float(sp32[1]), case["f"], lam.double())
    finally:
        torch.set_default_dtype(prev)
    r32 = orc.thin_lens(x, float(sp32[0]), float(sp32[1]), case["f"], lam)
    assert rel(lens, r64) <= max(4e-6, 2 * rel(r32, r64))  # 2.007e-6 drawn at a 45 x 2 field
    # aperture (a circle of radius >= half the smaller extent: the reference means to raise
    # ValueError there -- it builds one without raising and then fails on an unset radius -- and
    # this build raises it)
    circ_too_big = case["kind"] == "circ" and not (
        np.float32(case["size"]) < min(np.float32(dx) * np.float32(H), np.float32(dy) * np.float32(W)) / np.float32(2))
    if circ_too_big:
        with pytest.raises(ValueError):
            ApertureElement(case["kind"], case["size"])(ef(x.to(_dev())))
    else:
        ap = ApertureElement(case["kind"], case["size"])(ef(x.to(_dev()))).data
        mask = orc.aperture_mask(H, W, float(sp32[0]), float(sp32[1]), case["kind"], case["size"])
        assert torch.equal(ap.cpu(), x * mask)
    # resampler, forward and gradient
    Ho, Wo = case["Ho"], case["Wo"]
    dxo, dyo = dx / case["zoom"], dy / case["zoom"]
    xd = x.to(_dev()).requires_grad_(True)
    out = Field_Resampler(Ho, Wo, dxo, dyo)(ef(xd)).data
    gout = torch.randn(out.shape, dtype=torch.complex64, generator=g)
    gx, = torch.autograd.grad(out, xd, grad_outputs=gout.to(_dev()))
    def oracle_resample(dt):
        prev = torch.get_default_dtype()
        torch.set_default_dtype(torch.float64 if dt == torch.complex128 else torch.float32)
        try:
            xo = x.clone().to(dt).requires_grad_(True)
            ro = orc.resample(xo, [float(sp32[0]), float(sp32[1])], Ho, Wo, float(np.float32(dxo)),
                              float(np.float32(dyo)))
            rgx, = torch.autograd.grad(ro, xo, grad_outputs=gout.to(dt))
        finally:
            torch.set_default_dtype(prev)
        return ro.detach(), rgx

    r32, rg32 = oracle_resample(torch.complex64)
    r64, rg64 = oracle_resample(torch.complex128)
    assert tuple(out.shape) == tuple(r32.shape)
    if min(H, W) < 3:
        # the reference's grid normalisation divides by dx ((H - 1) // 2) = 0: NaN everywhere, as here
        assert bool(torch.isnan(r32).all()) and bool(torch.isnan(out).all())
        return
    # The sampling coordinates are fp32: the output grid linspace(-(n-1)//2, (n-1)//2, n) * d_out is
    # formed as torch's CUDA kernel forms it (start + step i from either end), torch's CPU kernel
    # (the oracle) in 8-wide vector chunks -- the same values up to an ulp or two of the grid value,
    # and -34 + step * 34 style sums turn that into ~1e-5 of a pixel.  A bilinear weight moves by at
    # most the coordinate error (in pixels), so each output may move by that times the sum of its
    # taps' magnitudes: 4 ulps of the largest grid value, scaled to input pixels, on each axis.
    def ulp_pix(n_out, d_out, norm, n_in):
        lmax = float((n_out - 1) // 2)                      # largest |linspace| value
        gmax = lmax * abs(d_out) / max(norm, 1e-30)         # ... in normalised grid units
        e_norm = 4.0 * float(np.spacing(np.float32(max(lmax, 1.0)))) * abs(d_out) / max(norm, 1e-30) \
            + 4.0 * float(np.spacing(np.float32(max(gmax, 1.0))))
        return e_norm * (n_in - 1) / 2.0                    # in input pixels

    dw = ulp_pix(Ho, dxo, float(np.float32(dx)) * ((H - 1) // 2), H) + ulp_pix(Wo, dyo, float(np.float32(dy)) * ((W - 1) // 2), W)
    bound = dw * 4 * float(x.abs().max()) + 1e-5 * r64.abs()
    assert bool(((out.detach().cpu().to(torch.complex128) - r64).abs() <= bound).all()), float(dw)
    gbound = dw * 4 * float(gout.abs().sum()) + 1e-5 * rg64.abs()
    assert bool(((gx.detach().cpu().to(torch.complex128) - rg64).abs() <= gbound).all())
