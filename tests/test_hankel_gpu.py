"""The Hankel propagator's kernels (csrc/thz_hankel.hip) against the fp64 restatement of the model on their own
exported table (tests/hankel_ref.py), held to parity.MARGIN x the fp32 floor of the same algebra."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import gpu_util, hankel_ref, parity

pytestmark = pytest.mark.gpu
LOG = "THZ_HANKEL_PARITY_LOG"
LAM = gpu_util.f32(1e-3)
C64, C128 = torch.complex64, torch.complex128

# (N, Z, B, C, keep).  N = 129 is the smallest size whose host plan splits K (HK_KMIN = 128: ranges of 96 and 33).
CASES = [(1, 1, 1, 1, 1), (31, 1, 1, 1, 31), (33, 3, 1, 1, 33), (64, 2, 1, 3, 1), (100, 3, 2, 1, 33),
         (129, 2, 1, 2, 129)]


@functools.lru_cache(maxsize=None)
def _case(case):
    """inputs, the exported table and H, the fp64 restatement and its fp32 floor -- computed once per case"""
    from quantizationawarethzdoe_amd import hankel
    N, Z, B, C, keep = case
    dev = gpu_util.dev()
    lams = [gpu_util.f32(LAM * s) for s in (1.0, 1.1, 0.9)[:C]]
    r_max = N * LAM / 4 if N == 64 else N * LAM  # N lambda / 4: the upper rings of kappa are evanescent
    zs = [gpu_util.f32(0.05 + 0.025 * i) for i in range(Z)]
    f = gpu_util.white_cpu((B, C, N), seed=N)
    T, w, zeros = (t.cpu() for t in hankel.hankel_table(N, dev))
    H = hankel.hankel_transfer_function(lams, r_max, zs, N, dev).cpu()
    ref = hankel_ref.forward(T, w, H, f, keep)
    floor = parity.floor_of(hankel_ref.forward(T, w, H, f, keep, C64), ref, rel_cap=1e-5, max_cap=1e-3,
                            at_least_u32=N == 1)
    return dict(dev=dev, lams=lams, r_max=r_max, zs=zs, f=f, T=T, w=w, zeros=zeros, H=H, ref=ref, floor=floor)


def _run(case, c, **kw):
    from quantizationawarethzdoe_amd import hankel
    return hankel.hankel_propagate(kw.pop("f", c["f"]).to(c["dev"]), c["lams"], c["r_max"], kw.pop("zs", c["zs"]),
                                   keep=kw.pop("keep", case[4]))


@pytest.mark.parametrize("case", CASES, ids=str)
def test_forward_parity(case):
    c = _case(case)
    parity.judge(LOG, "hankel", "forward", str(case), _run(case, c).cpu(), c["ref"], c["floor"])


@pytest.mark.parametrize("case", CASES[2:4], ids=str)
def test_transfer_function(case):
    """H is its fp64 formula rounded to complex64 to 2 ulp per component, zeros where kappa >= k"""
    c = _case(case)
    want = hankel_ref.transfer(c["zeros"], c["r_max"], c["lams"], c["zs"]).to(C64)
    got, want = torch.view_as_real(c["H"]), torch.view_as_real(want)
    ulp = torch.from_numpy(np.spacing(want.abs().numpy()))
    assert bool(((got - want).abs() <= 2 * ulp).all())
    assert bool(((got == 0) == (want == 0)).all())
    if case[0] == 64:
        assert bool((c["H"] == 0).any()) and bool((c["H"] != 0).any())


@pytest.mark.parametrize("case", [CASES[2], CASES[4]], ids=str)
def test_backward(case):
    """the profile's gradient of sum |out|^2 mask against fp64 autograd of the restatement, within MARGIN x the
    error of the complex64 CPU autograd; the adjoint identity <A x, y> = <x, A^H y> in fp64 to 1e-5"""
    c = _case(case)
    g = torch.Generator().manual_seed(7)
    mask = torch.rand(c["ref"].shape, generator=g)

    def cpu_grad(cdtype):
        x = c["f"].clone().to(cdtype).requires_grad_(True)  # a leaf of its own: the case is shared
        out = hankel_ref.forward(c["T"], c["w"], c["H"], x, case[4], cdtype)
        (out.abs().pow(2) * mask.to(out.real.dtype)).sum().backward()
        return x.grad.to(C128)

    x = c["f"].to(c["dev"]).requires_grad_(True)
    out = _run(case, c, f=x)
    (out.abs().pow(2) * mask.to(c["dev"])).sum().backward()
    g64, g32 = cpu_grad(C128), cpu_grad(C64)
    e32 = float((g32 - g64).norm() / g64.norm())
    err = float((x.grad.cpu().to(C128) - g64).norm() / g64.norm())
    parity.emit(LOG, f"hankel backward {case}: e32 {e32:.3e} err {err:.3e} ratio {err / e32:.2f}")
    assert err <= parity.MARGIN * e32

    y = gpu_util.white_cpu(tuple(c["ref"].shape), seed=11)
    x2 = c["f"].to(c["dev"]).requires_grad_(True)
    ax = _run(case, c, f=x2)
    ax.backward(y.to(c["dev"]))
    lhs = torch.vdot(ax.detach().cpu().to(C128).flatten(), y.to(C128).flatten())
    rhs = torch.vdot(c["f"].to(C128).flatten(), x2.grad.cpu().to(C128).flatten())
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs)


def test_bitwise():
    """a repeated call, graph replays against eager, Z planes against Z one-plane calls, keep = 33 against the
    first 33 entries of keep = N"""
    from quantizationawarethzdoe_amd.Props.Hankel_Prop import Hankel_prop
    case = CASES[4]
    N, Z, B, C, keep = case
    c = _case(case)
    eager = _run(case, c)
    assert gpu_util.bits(eager, _run(case, c))
    assert gpu_util.bits(eager, _run(case, c, keep=N)[..., :keep].contiguous())
    prop = Hankel_prop(0.0, N, c["r_max"], device=c["dev"])
    f = c["f"].to(c["dev"])
    for i, z in enumerate(c["zs"]):
        prop.z = z
        assert gpu_util.bits(prop.propagate_zr(f, c["lams"], c["zs"])[i], prop(f, c["lams"]))
    zdev = torch.tensor(c["zs"], dtype=torch.float32, device=c["dev"])
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        _run(case, c, f=f, zs=zdev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            out = _run(case, c, f=f, zs=zdev)  # the profile is on the device: no copy inside the capture
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert gpu_util.bits(eager, out)


def test_gaussian_beam_against_the_paraxial_formula():
    """the 8 mm Gaussian at N = 512, z = 50 mm: relative L2 against the paraxial beam within 2 x the 1.4e-4 of the
    fp64 restatement, which is the formula's own error; a complex128 profile is refused by name"""
    from quantizationawarethzdoe_amd import hankel
    dev = gpu_util.dev()
    N, r_max, w0, z = 512, 0.1, 8e-3, gpu_util.f32(0.05)
    r = hankel.hankel_nodes(N, r_max, dev)[0]
    beam = torch.exp(-(r / w0) ** 2).to(C128).view(1, 1, N)
    out = hankel.hankel_propagate(beam.to(C64), [LAM], r_max, [z])[0, 0, 0].cpu().to(C128)
    k, zr, r = 2 * math.pi / LAM, math.pi * w0 ** 2 / LAM, r.cpu()
    wz, rc, gouy = w0 * math.sqrt(1 + (z / zr) ** 2), z * (1 + (zr / z) ** 2), math.atan(z / zr)
    exact = (w0 / wz) * torch.exp(-(r / wz) ** 2) * torch.polar(torch.ones_like(r), k * z + k * r ** 2 / (2 * rc) - gouy)
    assert float((out - exact).norm() / exact.norm()) <= 2 * 1.4e-4
    with pytest.raises(TypeError, match="complex128"):
        hankel.hankel_propagate(beam.to(dev), [LAM], r_max, [z])
