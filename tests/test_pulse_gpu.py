"""The pulse kernels (csrc/thz_pulse.hip) against the fp64 restatement of the model on their own exported table
(tests/pulse_ref.py): the products held to parity.MARGIN x the fp32 floor of the same algebra, the maps and the gradients
by the rules of parity.Ratios."""
import functools
import math

import pytest
import torch

from tests import gpu_util, parity, pulse_ref

pytestmark = pytest.mark.gpu
LOG = "THZ_PULSE_PARITY_LOG"
C64, C128 = torch.complex64, torch.complex128
C0 = 299792458.0
RATIOS = parity.Ratios(LOG, "")

# (B, C, T, H, W).  A workgroup owns 128 pixels (32 per wave), a time tile is 32 samples, C <= 8 / <= 32 / <= 64 are three
# instantiations.  One element; an odd C on the C <= 8 form and a second wave of one pixel; a second time tile of one
# sample and two batch entries of 150 pixels (a second workgroup of 22 that must not run into the next entry); the largest
# C (two channel blocks of the adjoint); five time tiles on one workgroup, dealt to grid.y by the synthesis; one channel
# above the 32-channel form with a second workgroup of one pixel.
CASES = [(1, 1, 1, 1, 1), (1, 3, 5, 1, 33), (2, 32, 33, 3, 50), (1, 64, 2, 8, 8), (1, 2, 130, 1, 64), (1, 33, 40, 1, 129)]


def _axes(C, T, dt=0.25e-12):
    f = torch.linspace(0.2e12, 1.0e12, C, dtype=torch.float64) if C > 1 else torch.tensor([0.6e12], dtype=torch.float64)
    return (C0 / f).tolist(), ((torch.arange(T, dtype=torch.float64) - T / 2) * dt).tolist()


@functools.lru_cache(maxsize=None)
def _case(case):
    """inputs, the exported table, the fp64 restatements and their fp32 floors -- computed once per case"""
    from quantizationawarethzdoe_amd import pulse
    B, C, T, H, W = case
    dev = gpu_util.dev()
    lam, times = _axes(C, T)
    table = pulse.time_table(lam, times, weights="none", device=dev).cpu()
    U, g = gpu_util.white_cpu((B, C, H, W), seed=C + T), gpu_util.white_cpu((B, T, H, W), seed=H + W)
    syn, adj = pulse_ref.synthesize(table, U), pulse_ref.adjoint(table, g)
    # A sum of one to three complex products (C or, for the adjoint, T of them) rounds so few times that the complex64 CPU run can land below one rounding
    # in relative L2 (4.8e-8 for C = 3 here): floor_of refuses such a floor unless it may clamp it up to 2^-24, as the
    # Hankel and mode tests do for their one-term sums.
    caps = dict(rel_cap=1e-5, max_cap=1e-3, at_least_u32=min(C, T) <= 3)
    return dict(dev=dev, lam=lam, times=times, table=table, U=U, g=g, syn=syn, adj=adj,
                syn_floor=parity.floor_of(pulse_ref.synthesize(table, U, C64), syn, **caps),
                adj_floor=parity.floor_of(pulse_ref.adjoint(table, g, C64), adj, **caps))


def _synthesize(c, U):
    from quantizationawarethzdoe_amd import pulse
    return pulse.synthesize(U, c["times"], wavelengths=c["lam"], weights="none")


@pytest.mark.parametrize("case", CASES, ids=str)
def test_parity(case):
    c = _case(case)
    U = c["U"].to(c["dev"]).requires_grad_(True)
    E = _synthesize(c, U)
    parity.judge(LOG, "pulse", "synthesize", str(case), E.detach().cpu(), c["syn"], c["syn_floor"])
    E.backward(c["g"].to(c["dev"]))
    parity.judge(LOG, "pulse", "adjoint", str(case), U.grad.cpu(), c["adj"], c["adj_floor"])


@functools.lru_cache(maxsize=None)
def _pulses(kind):
    """200 delayed pulses U[c, p] = A_p exp(+i 2 pi f_c tau_p) + 0.02 white with tau_p = (j_p + 0.2 - T / 2) dt, so that
    the peak sample is j_p.  "wide": 32 channels 0.2 .. 1.0 THz under a Gaussian spectrum (0.6 THz, sigma 0.15 THz), 64
    samples of 0.5 ps.  "tails": C = 3 (0.2, 0.5, 1.0 THz: unequal steps, so three lines still make one sharp peak per
    10 ps), T = 33 samples of 0.25 ps -- an odd C, a one-sample time tail -- and an all-zero pixel."""
    from quantizationawarethzdoe_amd import pulse
    dev = gpu_util.dev()
    if kind == "wide":
        f, T, dt, hi = torch.linspace(0.2e12, 1.0e12, 32, dtype=torch.float64), 64, 0.5e-12, 55
        S = torch.exp(-(f - 0.6e12) ** 2 / (2 * 0.15e12 ** 2)).to(C128)
    else:
        f, T, dt, hi, S = torch.tensor([0.2e12, 0.5e12, 1.0e12], dtype=torch.float64), 33, 0.25e-12, 24, None
    lam, times = (C0 / f).tolist(), ((torch.arange(T, dtype=torch.float64) - T / 2) * dt).tolist()
    g = torch.Generator().manual_seed(5)
    A = 0.5 + torch.rand(200, generator=g, dtype=torch.float64)
    jp = torch.randint(8, hi + 1, (200,), generator=g)
    tau = (jp + 0.2 - T / 2) * dt
    U = A * torch.exp(2j * math.pi * f[:, None] * tau) + 0.02 * torch.randn(len(f), 200, dtype=C128, generator=g)
    if kind == "tails":
        U[:, 7], jp[7] = 0, 0
    U = U.to(C64)[None, :, None, :]
    table = pulse.time_table(lam, times, S, device=dev).cpu()
    t, w = (v.cpu() for v in pulse.time_samples(lam, times, S, device=dev))
    ref, j64 = pulse_ref.maps(table, t, w, U)
    # the precondition, before any kernel is looked at: both restatements find j_p, and no other sample comes near
    I = pulse_ref.synthesize(table, U).abs()[0, :, 0, :] ** 2
    top = I.topk(2, 0).values
    assert bool((j64 == pulse_ref.maps(table, t, w, U, torch.float32)[1]).all()) and bool((j64[0, 0] == jp).all())
    assert bool((top[1] <= 0.95 * top[0]).all())
    return dict(dev=dev, lam=lam, times=times, S=S, U=U, table=table, t=t, w=w, ref=ref)


def _maps(c, U):
    from quantizationawarethzdoe_amd import pulse
    return pulse.pulse_maps(U, c["times"], c["S"], wavelengths=c["lam"])


@pytest.mark.parametrize("kind", ["wide", "tails"])
def test_maps(kind):
    c = _pulses(kind)
    got = _maps(c, c["U"].to(c["dev"]))
    assert torch.equal(got.t_peak.cpu().double(), c["ref"][:, 2])
    for k, name in ((0, "energy"), (1, "peak"), (3, "t_mean"), (4, "t_rms")):
        RATIOS.value(name, kind, got[k], lambda dtype: pulse_ref.maps(c["table"], c["t"], c["w"], c["U"], dtype)[0][:, k])
    if kind == "tails":
        assert [float(m[0, 0, 7]) for m in got] == [0.0, 0.0, float(c["t"][0]), 0.0, 0.0]


def _grad(fn, x0, dtype):
    """view_as_real of the gradient of the real scalar fn(x, dtype) at x0 cast to the complex type of ``dtype``"""
    x = x0.clone().to(C128 if dtype == torch.float64 else C64).requires_grad_(True)
    fn(x, dtype).backward()
    return torch.view_as_real(x.grad)


@pytest.mark.parametrize("kind", ["wide", "tails"])
def test_backward_maps(kind):
    """sum_p (w1 energy + w2 peak + w3 t_mean + w4 t_rms), the weights seeded in 0.5 .. 1.5 over each map's mean size"""
    c = _pulses(kind)
    w = (0.5 + torch.rand(5, generator=torch.Generator().manual_seed(9), dtype=torch.float64)) / c["ref"].abs().mean((0, 2, 3))
    w[2] = 0

    def loss(x, dtype):
        return (pulse_ref.maps(c["table"], c["t"], c["w"], x, dtype)[0] * w.to(dtype)[None, :, None, None]).sum()

    x = c["U"].to(c["dev"]).requires_grad_(True)
    sum(wk.float() * m.sum() for wk, m in zip(w, _maps(c, x))).backward()
    RATIOS.grad("maps", kind, torch.view_as_real(x.grad), lambda dtype: _grad(loss, c["U"], dtype))


@pytest.mark.parametrize("case", [CASES[2], CASES[5]], ids=str)
def test_backward_synthesis(case):
    """the gradient of sum |E|^2 mask by the same rule, and the adjoint identity <A x, y> = <x, A^H y> in fp64 to 1e-5"""
    c = _case(case)
    mask = torch.rand(c["syn"].shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64)

    def loss(x, dtype):
        return (pulse_ref.synthesize(c["table"], x, x.dtype).abs().pow(2) * mask.to(dtype)).sum()

    x = c["U"].to(c["dev"]).requires_grad_(True)
    (_synthesize(c, x).abs().pow(2) * mask.float().to(c["dev"])).sum().backward()
    RATIOS.grad("synthesize", str(case), torch.view_as_real(x.grad), lambda dtype: _grad(loss, c["U"], dtype))

    x2 = c["U"].to(c["dev"]).requires_grad_(True)
    ax = _synthesize(c, x2)
    ax.backward(c["g"].to(c["dev"]))
    lhs = torch.vdot(ax.detach().cpu().to(C128).flatten(), c["g"].to(C128).flatten())
    rhs = torch.vdot(c["U"].to(C128).flatten(), x2.grad.cpu().to(C128).flatten())
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs)


def test_bitwise():
    """a repeated call, three graph replays against eager and B = 2 against the entries one at a time, for synthesize and
    pulse_maps; a complex128 field is refused by name"""
    from quantizationawarethzdoe_amd import pulse
    dev = gpu_util.dev()
    lam, times = _axes(9, 40)
    U = gpu_util.white_cpu((2, 9, 3, 50), seed=3).to(dev)

    def run(x):
        return (pulse.synthesize(x, times, wavelengths=lam),) + tuple(pulse.pulse_maps(x, times, wavelengths=lam))

    eager = run(U)
    assert all(gpu_util.bits(a, b) for a, b in zip(eager, run(U)))
    for b in range(2):
        assert all(gpu_util.bits(a[b], o[0]) for a, o in zip(eager, run(U[b:b + 1].contiguous())))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            out = run(U)  # the table exists: the capture only launches
    for _ in range(3):
        for o in out:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(gpu_util.bits(a, o) for a, o in zip(eager, out))
    with pytest.raises(TypeError, match="complex128"):
        pulse.pulse_maps(U.to(C128), times, wavelengths=lam)
    for what, (ratio, name) in sorted(RATIOS.worst.items()):
        parity.emit(LOG, f"pulse {what:<16s} {name:<26s} err / bound {ratio:.4f}")
