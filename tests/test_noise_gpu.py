"""The detector noise kernels on the GPU (thz_noise.hip through optics.add_noise / optics.detect and
the reference-named modules).

Formula parity is exact: the kernels export the draws they use (thz_noise_draws), tests/noise_ref.py
restates the reference's formulas on them in torch ops (pinned to the reference's own outputs by
tests/test_noise_cpu.py), and the two must agree bit for bit -- on an aligned pointer (16-byte
accesses) and on one offset by an element (element-width accesses), at sizes around the four-element
group, the 256-thread workgroup and the 1024-element chunk.  The samplers' laws are held to 5-sigma
moment bounds and a chi-square cap of dof + 6 sqrt(2 dof) by tests/noise_stats.py, which the CPU
suite first runs on torch's own samplers.

The SNR form's gradient is compared with torch autograd on the same formula and the exported draws:
relative L2 against the fp64 result <= 4 x the error of torch's own fp32 evaluation.  Measured on an
MI355X (profiles/noise_parity_ratios.txt; every case prints its line, THZ_NOISE_PARITY_LOG=<file>
appends them to a file).
"""
import math
import os

import numpy as np
import pytest
import torch

from quantizationawarethzdoe_amd import _lib, optics
from quantizationawarethzdoe_amd.Addons import Noise as A
from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
from quantizationawarethzdoe_amd.utils import Noise as U
from tests import noise_ref as nr
from tests import noise_stats as ns

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4, 5, 255, 256, 257, 1023, 4099)
SIGMA, AMP, SNR_DB = 0.25, 0.3, 12.0
N_STAT = 1 << 20


def _dev():
    return torch.device("cuda:0")


def _state(seed=1234, step=7):
    return torch.tensor([seed, step], dtype=torch.int32, device=_dev())


def _place(t, offset):
    """A contiguous device copy of ``t`` whose pointer is 16-byte aligned (offset 0) or one element
    past such an address (offset 1)."""
    buf = torch.empty(t.numel() + offset, dtype=t.dtype, device=_dev())
    assert buf.data_ptr() % 16 == 0
    v = buf[offset:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and (v.data_ptr() % 16 == 0) == (offset == 0)
    return v


def _inputs(n, offset, seed=0):
    g = torch.Generator().manual_seed(seed + n)
    return _place(torch.randn(n, generator=g), offset), _place(torch.view_as_complex(torch.randn(n, 2, generator=g)),
                                                               offset)


def _bits(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.is_complex():
        a, b = torch.view_as_real(a), torch.view_as_real(b)
    return bool((a.view(torch.int32) == b.view(torch.int32)).all())


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_formula_parity(n, offset):
    x, e = _inputs(n, offset)
    rng = (_state(), 5)
    nd, ud, cd = (optics.noise_draws(w, rng, n) for w in ("normal", "uniform", "complex_normal"))
    assert _bits(optics.add_noise(x, "gauss", sigma=SIGMA, rng=rng), nr.gauss(x, nd, SIGMA))
    assert _bits(optics.add_noise(x, "uniform", a=AMP, rng=rng), nr.uniform(x, ud, AMP))
    assert _bits(optics.add_noise(e, "gauss", sigma=SIGMA, rng=rng), nr.gauss(e, cd, SIGMA))
    inten = e.abs() ** 2
    assert _bits(optics.detect(e, "gauss", sigma=SIGMA, rng=rng), nr.gauss(inten, nd, SIGMA))
    assert _bits(optics.detect(e, "uniform", a=AMP, rng=rng), nr.uniform(inten, ud, AMP))
    # the Poisson kinds on a sample read back from the kernel: the gain / normalize bookkeeping, and that a
    # POISSON_GAUSS element's normal draw is the stream's own (the independence of the Poisson draws from it and
    # from the next stream's is test_poisson_streams_are_independent's)
    xp = x.abs() * 8
    counts = optics.add_noise(xp, "poisson", gain=0.5, normalize=False, rng=rng)
    assert _bits(optics.add_noise(xp, "poisson", gain=0.5, normalize=True, rng=rng), nr.poisson(xp, counts, 0.5, True))
    assert _bits(optics.add_noise(xp, "poisson_gauss", gain=0.5, sigma=SIGMA, rng=rng),
                 nr.poisson_gauss(xp, counts, nd, 0.5, SIGMA))


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_snr_form_scale_and_output(n, offset):
    rng = (_state(), 5)
    for x, what in zip(_inputs(n, offset), ("normal", "complex_normal")):
        scale = optics.signal_scale(x, 10 ** (SNR_DB / 10))
        want = np.float32(nr.snr_scale_fp64(x.cpu(), SNR_DB))
        assert abs(np.float64(scale.item()) - np.float64(want)) <= np.float64(np.spacing(want)), (scale.item(), want)
        assert _bits(optics.signal_scale(x, 10 ** (SNR_DB / 10)), scale)  # the same input gives the same bits
        draws = optics.noise_draws(what, rng, n)
        assert _bits(optics.add_noise(x, "gauss", snr_db=SNR_DB, rng=rng), nr.gauss(x, draws, scale))
        assert _bits(U.GaussianNoise(SNR_DB)(x, rng=rng), nr.gauss(x, draws, scale))


KINDS = (("gauss", dict(sigma=SIGMA)), ("uniform", dict(a=AMP)), ("poisson", dict(gain=0.5)),
         ("poisson_gauss", dict(gain=2.0, sigma=SIGMA)))


@pytest.mark.parametrize("kind,kw", KINDS)
def test_index_invariance(kind, kw):
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(4099, generator=g) * 30).to(_dev())  # rates on both sides of the sampler switch at 10
    state = _state()
    full = optics.add_noise(x, kind, rng=(state, 2), **kw)
    for k in (1, 5, 257):
        assert _bits(optics.add_noise(x[:k], kind, rng=(state, 2), **kw), full[:k]), k
    assert _bits(optics.add_noise(x, kind, rng=(state.clone(), 2), **kw), full)
    assert not _bits(optics.add_noise(x, kind, rng=(state, 3), **kw), full)
    assert not _bits(optics.add_noise(x, kind, rng=(_state(step=8), 2), **kw), full)
    assert not _bits(optics.add_noise(x, kind, rng=(_state(seed=1235), 2), **kw), full)


def test_default_state_follows_torch_seed():
    x = torch.ones(1000, device=_dev())
    torch.manual_seed(11)
    a = optics.add_noise(x, "gauss")
    b = optics.add_noise(x, "gauss")
    torch.manual_seed(11)
    assert _bits(optics.add_noise(x, "gauss"), a) and not _bits(a, b)


def test_normal_draws():
    rng = (_state(seed=20261020, step=0), 1)
    n = optics.noise_draws("normal", rng, N_STAT)
    c = optics.noise_draws("complex_normal", rng, N_STAT)
    assert _bits(c.real.contiguous(), n * 0.70710678118654752)  # a real draw is the pair's first output
    checks = ns.normal_checks(n, pair=c.imag, max_abs=5.78)
    print("normal draws:", {k: (float(f"{v[0]:.4g}"), float(f"{v[1]:.4g}")) for k, v in checks.items()})
    assert not ns.failures(checks), ns.failures(checks)
    bad = ns.failures(ns.normal_checks(c.imag * math.sqrt(2.0), max_abs=5.78))
    assert not bad, bad
    u = optics.noise_draws("uniform", rng, N_STAT)
    assert 0.0 <= float(u.min()) and float(u.max()) < 1.0 and abs(float(u.double().mean()) - 0.5) <= 5 / math.sqrt(12 * N_STAT)


def _poisson(lam_tensor, stream=4, **kw):
    return optics.add_noise(lam_tensor, "poisson", gain=1.0, normalize=False, rng=(_state(seed=99, step=3), stream), **kw)


@pytest.mark.parametrize("lam", [0.05, 0.9, 3.0, 9.99, 10.0, 37.5, 1000.0, 1e5])
def test_poisson_draws(lam):
    s = _poisson(torch.full((N_STAT,), lam, device=_dev()))
    checks = ns.poisson_checks(s, float(np.float32(lam)))
    print(f"poisson lam={lam}:", {k: (float(f"{v[0]:.4g}"), float(f"{v[1]:.4g}")) for k, v in checks.items()})
    assert not ns.failures(checks), ns.failures(checks)


@pytest.mark.parametrize("lam", [3.0, 10.0, 37.5])
@pytest.mark.parametrize("stream", [0, 1, 6])
def test_poisson_streams_are_independent(lam, stream):
    """Streams s and s + 1 of one state at an equal rate (even and odd s; the rejection sampler at 10
    and 37.5, the inversion at 3): no shared attempt words -- correlation and the fraction of equal
    counts at their laws.  And a stream's Poisson counts against the same stream's normal draws
    (the two draws of a POISSON_GAUSS element)."""
    x = torch.full((N_STAT,), lam, device=_dev())
    a, b = _poisson(x, stream=stream), _poisson(x, stream=stream + 1)
    checks = ns.poisson_pair_checks(a, b, float(np.float32(lam)))
    nd = optics.noise_draws("normal", (_state(seed=99, step=3), stream), N_STAT)
    checks["normal"] = (abs(ns.corr(a, nd)), 5 / math.sqrt(N_STAT))
    print(f"poisson streams {stream}, {stream + 1} lam={lam}:",
          {k: (float(f"{v[0]:.4g}"), float(f"{v[1]:.4g}")) for k, v in checks.items()})
    assert not ns.failures(checks), ns.failures(checks)


def test_poisson_edge_rates_and_ramp():
    dev = _dev()
    assert not bool(_poisson(torch.zeros(4099, device=dev)).any())
    assert bool(torch.isnan(_poisson(torch.full((4099,), -1.0, device=dev))).all())
    assert bool(torch.isnan(_poisson(torch.full((4099,), float("nan"), device=dev))).all())
    mixed = _poisson(torch.tensor([0.0, -1.0, 5.0, float("nan"), 50.0], device=dev))
    assert mixed[0] == 0 and torch.isnan(mixed[1]) and torch.isnan(mixed[3]) and mixed[2] >= 0 and mixed[4] >= 0
    # every rate from 0 to 200 in one launch: both samplers inside each wave
    lam = torch.linspace(0, 200, N_STAT, device=dev)
    lam = lam[torch.randperm(N_STAT, device=dev, generator=torch.Generator(device=dev).manual_seed(0))].contiguous()
    s = _poisson(lam).double()
    assert bool(((s >= 0) & (s == s.floor())).all())
    edges = torch.linspace(0, 200, 9)
    for b in range(8):
        m = (lam >= edges[b]) & ((lam < edges[b + 1]) | (b == 7))
        dev_sum = float((s[m] - lam[m].double()).sum())
        assert abs(dev_sum) <= 5 * math.sqrt(float(lam[m].double().sum())), (b, dev_sum)


def test_gain_and_normalize():
    N = 1 << 18
    x = torch.full((N,), 3.0, device=_dev())
    rng = (_state(), 9)
    y = A.PoissonNoise(gain=0.5)(x, rng=rng).double()  # 0.5 P(6)
    assert bool(((y * 2) == (y * 2).floor()).all()) and bool((y >= 0).all())
    assert abs(float(y.mean()) - 3.0) <= 5 * math.sqrt(0.25 * 6.0 / N)
    c = A.PoissonNoise(gain=0.5, normalize=False)(x, rng=rng).double()
    assert bool((c == c.floor()).all()) and abs(float(c.mean()) - 6.0) <= 5 * math.sqrt(6.0 / N)
    assert _bits((c * 0.5).float(), y.float())


def _modules():
    return (A.GaussianNoise(SIGMA), A.UniformNoise(AMP), A.PoissonNoise(0.5), A.PoissonGaussianNoise(2.0, SIGMA))


def test_measure_equals_forward_on_the_intensity():
    g = torch.Generator().manual_seed(5)
    data = (3 * torch.view_as_complex(torch.randn(3, 2, 33, 35, 2, generator=g))).to(_dev())
    rng = (_state(), 6)
    for m in _modules():
        fused = m.measure(data, rng=rng)
        assert fused.dtype == torch.float32 and fused.shape == data.shape
        assert _bits(fused, m(data.abs() ** 2, rng=rng)), type(m).__name__
    field = ElectricField(data, wavelengths=[1e-3, 0.9e-3], spacing=1e-3, device=_dev())
    assert _bits(A.PoissonGaussianNoise(2.0, SIGMA).measure(field, rng=rng),
                 A.PoissonGaussianNoise(2.0, SIGMA)(data.abs() ** 2, rng=rng))
    assert _bits(U.GaussianNoise(SNR_DB).measure(field, rng=rng), U.GaussianNoise(SNR_DB)(data.abs() ** 2, rng=rng))


def test_pass_through_and_zero_gradients():
    g = torch.Generator().manual_seed(6)
    x0 = (torch.rand(4099, generator=g) * 20).to(_dev())
    gout = torch.randn(4099, generator=g).to(_dev())
    rng = (_state(), 1)
    for m in _modules():
        x = x0.clone().requires_grad_(True)
        m(x, rng=rng).backward(gout)
        want = gout if isinstance(m, (A.GaussianNoise, A.UniformNoise)) else torch.zeros_like(gout)
        assert _bits(x.grad, want), type(m).__name__
    e0 = torch.view_as_complex(torch.randn(4099, 2, generator=g)).to(_dev())
    for m in _modules():
        e = e0.clone().requires_grad_(True)
        m.measure(e, rng=rng).backward(gout)
        want = 2 * gout * e0 if isinstance(m, (A.GaussianNoise, A.UniformNoise)) else torch.zeros_like(e0)
        assert _bits(e.grad, want), type(m).__name__
    xc = e0.clone().requires_grad_(True)
    gc = torch.view_as_complex(torch.randn(4099, 2, generator=g)).to(_dev())
    A.GaussianNoise(SIGMA)(xc, rng=rng).backward(gc)
    assert _bits(xc.grad, gc)


def _rel(a, b):
    return float((a.to(b.dtype) - b).norm() / b.norm())


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex64"])
def test_snr_gradient_against_autograd(cplx):
    n = 4099
    x0 = _inputs(n, 0, seed=7)[1 if cplx else 0]
    gout = _inputs(n, 0, seed=8)[1 if cplx else 0]
    rng = (_state(), 5)
    draws = optics.noise_draws("complex_normal" if cplx else "normal", rng, n)
    snr = 10 ** (SNR_DB / 10)

    def autograd(dtype):
        x = x0.detach().to(dtype).clone().requires_grad_(True)
        y = x + draws.to(dtype) * torch.sqrt(torch.mean(x.abs() ** 2) / snr)
        y.backward(gout.to(dtype))
        return x.grad
    g64 = autograd(torch.complex128 if cplx else torch.float64)
    g32 = autograd(x0.dtype)
    x = x0.clone().requires_grad_(True)
    optics.add_noise(x, "gauss", snr_db=SNR_DB, rng=rng).backward(gout)
    floor, got = _rel(g32, g64), _rel(x.grad, g64)
    # the scale's term alone (grad - g), so the comparison is not dominated by the pass-through part
    floor_t, got_t = _rel(g32 - gout, g64 - gout.to(g64.dtype)), _rel(x.grad - gout, g64 - gout.to(g64.dtype))
    line = (f"snr_gradient {'complex64' if cplx else 'float32'} n={n}: rel-L2 vs fp64 autograd {got:.3e}, torch fp32 "
            f"{floor:.3e}, ratio {got / floor:.3f}; scale term alone {got_t:.3e} / {floor_t:.3e}")
    print(line)
    log = os.environ.get("THZ_NOISE_PARITY_LOG")
    if log:
        with open(log, "a") as f:
            f.write(line + "\n")
    assert got <= 4 * floor, line


def test_graph_replay_draws_afresh():
    dev = _dev()
    x = torch.linspace(0, 30, 4099, device=dev)
    state = _state()
    state0 = state.clone()
    one = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    noise = A.PoissonGaussianNoise(2.0, SIGMA)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        noise(x, rng=(state, 3))  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = noise(x, rng=(state, 3))
    graph.replay()
    first = y.clone()
    state.add_(one)  # the host's per-step advance, on the device
    graph.replay()
    second = y.clone()
    assert not _bits(first, second)
    state.copy_(state0)
    graph.replay()
    assert _bits(y, first)
    assert _bits(noise(x, rng=(state0, 3)), first)  # and the eager call agrees with the replay


NOISE_TIMERS = ("noise_apply", "noise_draws", "signal_scale_part", "signal_scale_finish", "snr_noise_bwd_part",
                "snr_noise_bwd_finish", "snr_noise_bwd")


def test_fallbacks():
    dev = _dev()
    x64 = torch.rand(257, dtype=torch.float64, device=dev) * 20
    e128 = torch.randn(257, dtype=torch.complex128, device=dev)
    _lib.timing_enable(True)
    try:
        _lib.timing_reset()
        for kind, kw in KINDS:
            assert optics.add_noise(x64, kind, **kw).dtype == torch.float64
            assert optics.detect(e128, kind, **kw).dtype == torch.float64
        assert optics.add_noise(e128, "gauss").dtype == torch.complex128
        assert optics.add_noise(x64, "gauss", snr_db=10).dtype == torch.float64
        y = optics.add_noise(x64.clone().requires_grad_(True), "gauss", snr_db=10)
        y.sum().backward()
        assert [_lib.timing_read(t)[1] for t in NOISE_TIMERS] == [0] * len(NOISE_TIMERS)
        xr = x64.float().requires_grad_(True)
        optics.add_noise(xr, "gauss", snr_db=10).sum().backward()
        assert [_lib.timing_read(t)[1] for t in NOISE_TIMERS] == [1, 0, 1, 1, 1, 1, 1]
    finally:
        _lib.timing_enable(False)
        _lib.timing_reset()
    with pytest.raises(TypeError):
        optics.add_noise(e128.to(torch.complex64), "uniform", a=AMP)
    with pytest.raises(TypeError):
        optics.add_noise(x64.half(), "gauss")
