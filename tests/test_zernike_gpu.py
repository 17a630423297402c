"""The Zernike kernels (csrc/thz_zernike.hip): the exported table against the fp64 closed form, the products against
fp64 algebra on that table, the fit, the element's gradient and the bits (tests/zernike_ref.py, tests/parity.py)."""
import functools

import pytest
import torch

from tests import gpu_util, parity, zernike_ref

pytestmark = pytest.mark.gpu
LOG = "THZ_ZERNIKE_PARITY_LOG"
RATIOS = parity.Ratios(LOG, "")
DX = 0.5e-3

# (H, W, R, (cx, cy), n_max, B, dy / dx), R and the centre in pixels of pitch dx.  All four K tiles off centre; K = 1;
# K = 36, one past a tile, on odd sizes and misaligned rows with dx != dy; a second 64-pixel segment, more than one
# workgroup and a second plane chunk; one pixel; a pupil cut by the grid (products only: its Gram's condition number
# is 1.2e4); 768 strips > ZK_PMAX = 512 partials and 2400 > ZK_SYN_GRID = 2048 synthesis strips, so that a workgroup
# walks several.
CASES = [(40, 48, 17.3, (1.7, -0.6), 14, 3, 1.0), (40, 48, 17.3, (1.7, -0.6), 0, 1, 1.0),
         (33, 31, 9.5, (0.3, 0.2), 7, 1, 0.8), (130, 70, 30.2, (2.2, -3.1), 14, 33, 1.0), (1, 1, 0.6, (0, 0), 0, 1, 1.0),
         (64, 64, 40, (0, 0), 10, 2, 1.0), (600, 200, 95.0, (3.0, -40.0), 4, 2, 1.0)]
FIT_CASES = [c for c in CASES if c[:2] != (64, 64)]
COND_CAP = 20.0


def _geo(case):
    H, W, R, (cx, cy), n, B, ratio = case
    return (H, W), (DX, ratio * DX), (cx * DX, cy * ratio * DX, R * DX)


def _floor(lo, ref, tiny):
    """parity.floor_of; a K = 1 or one-pixel product is exact in fp32, and that zero floor is clamped up to 2^-24"""
    if tiny and parity.errors(lo, ref)[0] == 0:
        return parity.U32, parity.U32
    return parity.floor_of(lo, ref, rel_cap=1e-5, max_cap=1e-3, at_least_u32=tiny)


@functools.lru_cache(maxsize=None)
def _case(case):
    """inputs, the exported table, the fp64 restatements on it and their fp32 floors -- computed once per case"""
    from quantizationawarethzdoe_amd import zernike
    shape, spacing, pupil = _geo(case)
    n, B = case[4], case[5]
    dev = gpu_util.dev()
    T = zernike.zernike_table(shape, spacing, pupil, n, dev).cpu()
    g = torch.Generator().manual_seed(case[0] + case[1])
    w = torch.randn(B, *shape, generator=g, dtype=torch.float64).float()
    a = torch.randn(B, T.shape[0], generator=g, dtype=torch.float64).float()
    ref = dict(project=zernike_ref.project(T, w), gram=zernike_ref.gram(T), synthesize=zernike_ref.synthesize(T, a))
    tiny = T.shape[0] == 1 or shape == (1, 1)
    lo = dict(project=zernike_ref.project(T, w, torch.float32), gram=zernike_ref.gram(T, torch.float32),
              synthesize=zernike_ref.synthesize(T, a, torch.float32))
    return dict(dev=dev, T=T, w=w, a=a, ref=ref, floor={k: _floor(lo[k], ref[k], tiny) for k in ref})


def _run(case, what, x=None):
    from quantizationawarethzdoe_amd import zernike
    shape, spacing, pupil = _geo(case)
    if what == "synthesize":
        return zernike.synthesize(x, shape, spacing, pupil)
    if what == "gram":
        return zernike.gram(shape, spacing, pupil, case[4], gpu_util.dev())
    return getattr(zernike, what)(x, spacing, pupil, case[4])


@pytest.mark.parametrize("case", CASES, ids=str)
def test_table(case):
    """the exported table against the fp64 recurrence (itself within 1e-9 of the explicit sum) by the Ratios.value
    rule, e32 the all-fp32 recurrence's error: 3.1e-5 at n = 14 on 40 x 48; exact zeros outside the pupil"""
    shape, spacing, pupil = _geo(case)
    T = _case(case)["T"]
    r64 = zernike_ref.recurrence(shape, spacing, pupil, case[4], torch.float64)
    assert float((r64 - zernike_ref.closed_form(shape, spacing, pupil, case[4])).abs().max()) <= 1e-9
    assert bool((T[:, ~zernike_ref.geometry(shape, spacing, pupil)[2]] == 0).all())
    RATIOS.value("table", str(case), T, lambda dt: zernike_ref.recurrence(shape, spacing, pupil, case[4], dt))


@pytest.mark.parametrize("case", CASES, ids=str)
def test_products(case):
    c = _case(case)
    G = _run(case, "gram")
    assert gpu_util.bits(G, G.T.contiguous())
    got = dict(project=_run(case, "project", c["w"].to(c["dev"])), gram=G,
               synthesize=_run(case, "synthesize", c["a"].to(c["dev"])))
    for what in ("project", "gram", "synthesize"):
        parity.judge(LOG, "zernike", what, str(case), got[what].cpu(), c["ref"][what], c["floor"][what], widths=(12, 60))


@pytest.mark.parametrize("case", [CASES[0], CASES[3]], ids=str)
def test_gradients(case):
    """the gradients of sum mask out^2 through both directions against autograd of the restatement"""
    c = _case(case)
    for what, x0, fn in (("project", c["w"], zernike_ref.project), ("synthesize", c["a"], zernike_ref.synthesize)):
        mask = torch.rand(c["ref"][what].shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64)

        def cpu_grad(dtype):
            x = x0.clone().to(dtype).requires_grad_(True)  # a leaf of its own: the case is shared
            (fn(c["T"], x, dtype).pow(2) * mask.to(dtype)).sum().backward()
            return x.grad

        x = x0.to(c["dev"]).requires_grad_(True)
        (_run(case, what, x).pow(2) * mask.float().to(c["dev"])).sum().backward()
        RATIOS.grad(what, str(case), x.grad, cpu_grad)


@pytest.mark.parametrize("case", FIT_CASES, ids=str)
def test_fit(case):
    c = _case(case)
    cond = float(torch.linalg.cond(c["ref"]["gram"]))
    parity.emit(LOG, f"zernike fit cond {case}: {cond:.3g}")
    assert cond <= COND_CAP
    RATIOS.value("fit", str(case), _run(case, "fit", c["w"].to(c["dev"])),
                 lambda dt: zernike_ref.solve(c["T"], c["w"], dt))


def test_element():
    """the gradient of a scalar loss through ZernikeDOEElement -> doe.modulate to the coefficients, against autograd
    through FixDOEElement on the map synthesised on the CPU (wrapped, so that the modulo's gradient is in it)"""
    from quantizationawarethzdoe_amd.Components.QuantizedDOE import FixDOEElement
    from quantizationawarethzdoe_amd.Components.ZernikeDOE import ZernikeDOEElement
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    case = CASES[0]
    c = _case(case)
    shape, spacing, pupil = _geo(case)
    lam, material, wrap, base = [gpu_util.lam_ghz(300.0)], [2.66, 0.03], 1.2e-3, 0.3e-3
    coeffs = 1e-4 * c["a"][0]
    U = gpu_util.white_cpu((1, 1) + shape, seed=5).to(c["dev"])
    mask = torch.rand(shape, generator=torch.Generator().manual_seed(9)).to(c["dev"])

    def loss(elem):
        field = ElectricField(U.clone(), wavelengths=lam[0], spacing=list(spacing), device=c["dev"])
        return (elem(field).data.abs().pow(2) * mask).sum()

    p = torch.nn.Parameter(coeffs.to(c["dev"]))
    loss(ZernikeDOEElement(p, pupil, shape, spacing, material, wrap=wrap, base=base, device=c["dev"])).backward()

    def ref_grad(dtype):
        a = coeffs.clone().to(dtype).requires_grad_(True)
        h = torch.remainder(base + zernike_ref.synthesize(c["T"], a[None], dtype)[0], wrap)
        fix = FixDOEElement(h.detach().float(), tolerance=0.0, material=material, device=c["dev"])
        loss(fix).backward()
        h.backward(fix.height_map.grad.cpu().to(dtype))
        return a.grad

    RATIOS.grad("element", str(case), p.grad, ref_grad)


def test_bitwise():
    """a repeated call, three graph replays against eager, and B = 33 planes against the planes one at a time"""
    case = CASES[3]
    c = _case(case)
    w, a = c["w"].to(c["dev"]), c["a"].to(c["dev"])
    eager = _run(case, "project", w), _run(case, "synthesize", a)
    assert gpu_util.bits(eager[0], _run(case, "project", w)) and gpu_util.bits(eager[1], _run(case, "synthesize", a))
    for b in range(w.shape[0]):
        assert gpu_util.bits(eager[0][b], _run(case, "project", w[b:b + 1].contiguous())[0])
        assert gpu_util.bits(eager[1][b], _run(case, "synthesize", a[b:b + 1].contiguous())[0])
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            out = _run(case, "project", w), _run(case, "synthesize", a)
    for _ in range(3):
        out[0].zero_(), out[1].zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert gpu_util.bits(eager[0], out[0]) and gpu_util.bits(eager[1], out[1])
    for what, (ratio, name) in sorted(RATIOS.worst.items()):
        parity.emit(LOG, f"zernike {what:<16s} {name:<60s} err / bound {ratio:.4f}")
