"""Time-domain THz pulses: what a THz time-domain system measures, the field against time at each detector pixel, from
the per-frequency phasors of a broadband ``ElectricField`` -- a module of this port alone like ifta.py, hankel.py and
modes.py (csrc/thz_pulse.hip).  The model is stated in include/thzdoe.h:

    Phi[j, c] = q_c S_c exp(-i 2 pi f_c t_j),    E[b, j, h, w] = sum_c Phi[j, c] U[b, c, h, w]

with the source spectrum S_c, quadrature weights q_c over the channel frequencies f_c = c0 / lambda_c and time samples
t_j.  ``synthesize`` writes E; ``pulse_maps`` writes five floats per pixel (energy, peak, t_peak, t_mean, t_rms) without
E ever reaching memory.  Both are products on the fp32 matrix cores, differentiable to the field.

Aliasing: a signal synthesised from discrete channels repeats with period 1 / df, so the time window
t_{T-1} - t_0 must be shorter than 1 / max df of the (sorted) channel list; a window that is not gets one warning.

``times`` (seconds, strictly increasing), ``wavelengths``, ``spectrum`` and ``weights`` are host numbers (a device
tensor would be read back).  The first call for a set of them builds the table on the host in fp64 and copies it -- a
blocking step, not capturable; every later call only launches: no sync, no torch compute kernel, capturable in
torch.cuda.graph.  A repeated call gives the same bits, and B entries in one call the bits of the entries one at a time.
"""
import collections
import math
import warnings

import torch

from . import _lib
from ._call import _require_device, call

C0 = 299792458.0  # m / s, exact (donn.py keeps 2.998e8 for its own purposes)

PulseMaps = collections.namedtuple("PulseMaps", "energy peak t_peak t_mean t_rms")
_TABLES = {}  # (frequencies, times, spectrum, weights, device index) -> (table, times, dt) on the device
_warned = []


def _host(v, dtype=torch.float64):
    return torch.as_tensor(v).detach().to("cpu", dtype).reshape(-1)


def _frequencies(wavelengths, frequencies, who):
    if (wavelengths is None) == (frequencies is None):
        raise ValueError(f"{who}: give wavelengths or frequencies=")
    f = _host(frequencies) if wavelengths is None else C0 / _host(wavelengths)
    if f.numel() < 1 or f.numel() > _lib.THZ_MAX_WAVELENGTHS or not bool((f > 0).all() and torch.isfinite(f).all()):
        raise ValueError(f"{who}: 1 .. {_lib.THZ_MAX_WAVELENGTHS} positive channel frequencies; got {f.tolist()}")
    return f


def trapezoid_weights(x):
    """the trapezoid weights of the float64 list ``x`` taken in ascending order, returned in the list's own order;
    1 for a single entry"""
    n = x.numel()
    if n == 1:
        return torch.ones(1, dtype=torch.float64)
    s, order = torch.sort(x)
    w = torch.empty(n, dtype=torch.float64)
    w[0], w[-1] = (s[1] - s[0]) / 2, (s[-1] - s[-2]) / 2
    w[1:-1] = (s[2:] - s[:-2]) / 2
    out = torch.empty_like(w)
    out[order] = w
    return out


def gaussian_spectrum(wavelengths, center_frequency, fwhm, chirp=0.0):
    """A Gaussian source spectrum on the channels of ``wavelengths`` -> complex128 [C] on the host (no kernel):
    |S_c|^2 has the full width at half maximum ``fwhm`` (Hz) about ``center_frequency`` (Hz), and ``chirp`` (s^2, a
    group-delay dispersion) adds the phase chirp (2 pi (f - f0))^2 / 2 -- with exp(-i omega t), a positive chirp makes
    the high frequencies arrive later."""
    f = C0 / _host(wavelengths)
    d = f - float(center_frequency)
    return torch.polar(torch.exp(-2.0 * math.log(2.0) * (d / float(fwhm)) ** 2), 0.5 * float(chirp) * (2 * math.pi * d) ** 2)


def _build(f, t, spectrum, weights, device, who):
    C, T = f.numel(), t.numel()
    if not 1 <= T <= _lib.PULSE_MAX_T:
        raise ValueError(f"{who}: 1 .. {_lib.PULSE_MAX_T} time samples; got {T}")
    if T > 1 and not bool((t[1:] > t[:-1]).all()):
        raise ValueError(f"{who}: the time samples must be strictly increasing")
    S = torch.ones(C, dtype=torch.complex128) if spectrum is None else _host(spectrum, torch.complex128)
    if isinstance(weights, str) or weights is None:
        if weights not in ("trapezoid", "none", None):
            raise ValueError(f"{who}: weights is 'trapezoid', 'none' or a list [C]; got {weights!r}")
        q = trapezoid_weights(f) if weights == "trapezoid" else torch.ones(C, dtype=torch.float64)
    else:
        q = _host(weights)
    if S.numel() != C or q.numel() != C:
        raise ValueError(f"{who}: {S.numel()} spectrum values and {q.numel()} weights for {C} channels")
    if C > 1 and T > 1 and not _warned:
        df = torch.sort(f)[0].diff().max()
        if float(t[-1] - t[0]) * float(df) >= 1.0:
            _warned.append(True)
            warnings.warn(f"{who}: the time window {float(t[-1] - t[0]):.3e} s is not shorter than 1 / max df = "
                          f"{1 / float(df):.3e} s: the synthesised signal repeats inside it")
    x = t[:, None] * f[None, :]          # cycles, fp64
    x = x - torch.round(x)               # reduced to [-1/2, 1/2] before the 2 pi
    table = ((q * S)[None, :] * torch.polar(torch.ones_like(x), -2.0 * math.pi * x)).to(torch.complex64)
    return (table.to(device), t.to(torch.float32).to(device), trapezoid_weights(t).to(torch.float32).to(device))


def _tables(wavelengths, times, spectrum, weights, device, frequencies=None, who="time_table"):
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"{who}: the MI355X path needs a ROCm device (got device {device}); "
                           "this framework has no CPU compute path")
    f, t = _frequencies(wavelengths, frequencies, who), _host(times)
    S = None if spectrum is None else tuple(_host(spectrum, torch.complex128).tolist())
    q = weights if isinstance(weights, str) or weights is None else tuple(_host(weights).tolist())
    index = device.index if device.index is not None else torch.cuda.current_device()
    key = (tuple(f.tolist()), tuple(t.tolist()), S, q, index)
    if key not in _TABLES:
        _TABLES[key] = _build(f, t, spectrum, weights, device, who)
    return _TABLES[key]


def time_table(wavelengths=None, times=None, spectrum=None, weights="trapezoid", device="cuda", frequencies=None):
    """Phi complex64 [T, C] on ``device``, exactly what the kernels apply: q_c S_c exp(-i 2 pi f_c t_j) with
    f_c = c0 / lambda_c (or ``frequencies=`` in Hz in place of ``wavelengths``), the phase formed and reduced in fp64 and
    the product rounded once to fp32.  ``spectrum`` complex [C] defaults to 1; ``weights`` is "trapezoid" (in frequency
    over the sorted channels, 1 for C = 1), "none" or a list [C]."""
    return _tables(wavelengths, times, spectrum, weights, device, frequencies)[0]


def time_samples(wavelengths=None, times=None, spectrum=None, weights="trapezoid", device="cuda", frequencies=None):
    """(times, dt) float32 [T] on ``device`` as the map kernels read them: the samples rounded to fp32 and their
    trapezoid weights (1 for T = 1)."""
    return _tables(wavelengths, times, spectrum, weights, device, frequencies)[1:]


def _as_field(field, wavelengths, who):
    if not torch.is_tensor(field) and hasattr(field, "data"):
        wavelengths = field.wavelengths_host if wavelengths is None else wavelengths
        field = field.data
    if not torch.is_tensor(field):
        raise TypeError(f"{who}: the field must be a tensor or an ElectricField")
    _require_device(field, who)
    if field.dtype == torch.complex128:
        raise TypeError(f"{who}: the kernels compute in complex64; got a complex128 field -- cast it, an fp64 "
                        "variant does not exist")
    if field.dtype != torch.complex64 or field.dim() != 4:
        raise TypeError(f"{who}: the field is complex64 [B, C, H, W]; got {field.dtype} {tuple(field.shape)}")
    if wavelengths is None:
        raise ValueError(f"{who}: a tensor needs wavelengths=")
    return field, wavelengths


def _desc(shape, T):
    B, C, H, W = shape
    return _lib.PulseDesc(B=B, C=C, T=T, H=H, W=W)


class _Synthesize(torch.autograd.Function):
    """E of thz_pulse_synthesize; the product is linear, so the backward is thz_pulse_adjoint."""

    @staticmethod
    def forward(ctx, field, table):
        ctx.table, ctx.shape = table, tuple(field.shape)
        B, C, H, W = field.shape
        out = torch.empty(B, table.shape[0], H, W, dtype=torch.complex64, device=field.device)
        call(_lib.lib().thz_pulse_synthesize, _desc(field.shape, table.shape[0]), field.contiguous(), table, out,
             device=field.device)
        return out

    @staticmethod
    def backward(ctx, g):
        return _Adjoint.apply(g.resolve_conj(), ctx.table, ctx.shape), None


class _Adjoint(torch.autograd.Function):
    """Ubar of thz_pulse_adjoint; its backward is thz_pulse_synthesize."""

    @staticmethod
    def forward(ctx, g, table, shape):
        ctx.table = table
        out = torch.empty(shape, dtype=torch.complex64, device=g.device)
        call(_lib.lib().thz_pulse_adjoint, _desc(shape, table.shape[0]), g.contiguous(), table, out, device=g.device)
        return out

    @staticmethod
    def backward(ctx, g):
        return _Synthesize.apply(g.resolve_conj(), ctx.table), None, None


class _Maps(torch.autograd.Function):
    """the five maps of thz_pulse_maps as one [B, 5, H, W] tensor; the backward is thz_pulse_maps_backward on the
    saved field and maps"""

    @staticmethod
    def forward(ctx, field, table, times, dt):
        B, C, H, W = field.shape
        field = field.contiguous()
        maps = torch.empty(B, 5, H, W, dtype=torch.float32, device=field.device)
        call(_lib.lib().thz_pulse_maps, _desc(field.shape, table.shape[0]), field, table, times, dt, maps,
             device=field.device)
        ctx.save_for_backward(field, maps)
        ctx.tables = (table, times, dt)
        return maps

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        field, maps = ctx.saved_tensors
        table, times, dt = ctx.tables
        out = torch.empty_like(field)
        call(_lib.lib().thz_pulse_maps_backward, _desc(field.shape, table.shape[0]), field, table, times, dt, maps,
             g.contiguous(), out, device=field.device)
        return out, None, None, None


def synthesize(field, times, spectrum=None, wavelengths=None, weights="trapezoid"):
    """The analytic signal of a broadband field: ``field`` an ElectricField (data and wavelengths) or a complex64
    [B, C, H, W] tensor with ``wavelengths=`` -> complex64 [B, T, H, W], E[b, j] = sum_c Phi[j, c] U[b, c] at the
    samples ``times`` (thz_pulse_synthesize, on the table of ``time_table``); its real part is the measured field.
    Mind the aliasing rule of the module's docstring.  Gradients flow to the field (thz_pulse_adjoint).  The output is
    T / C times the field: ``pulse_maps`` gives the pulse's figures of merit without it."""
    who = "synthesize"
    x, lam = _as_field(field, wavelengths, who)
    table = _tables(lam, times, spectrum, weights, x.device, who=who)[0]
    return _Synthesize.apply(x.resolve_conj(), table)


def pulse_maps_tensor(field, times, spectrum=None, wavelengths=None, weights="trapezoid"):
    """``pulse_maps`` as one float32 [B, 5, H, W] tensor in the order (energy, peak, t_peak, t_mean, t_rms)"""
    who = "pulse_maps"
    x, lam = _as_field(field, wavelengths, who)
    table, t, dt = _tables(lam, times, spectrum, weights, x.device, who=who)
    return _Maps.apply(x.resolve_conj(), table, t, dt)


def pulse_maps(field, times, spectrum=None, wavelengths=None, weights="trapezoid"):
    """The pulse at every pixel in five numbers, a named tuple of float32 [B, H, W] (thz_pulse_maps): ``energy`` =
    sum_j |E_j|^2 dt_j, ``peak`` = max_j |E_j|^2, ``t_peak`` the first sample that reaches it (the pulse front),
    ``t_mean`` the intensity-weighted arrival time and ``t_rms`` the rms duration; dt_j are the trapezoid weights of
    ``times``.  A dark pixel (energy 0) has t_mean = t_rms = 0 and t_peak = t_0.  The time-resolved field is never
    written: the call allocates the five maps.  Gradients flow to the field through thz_pulse_maps_backward (t_peak
    carries none), so ``-maps.peak[..., r, c]`` is an objective for broadband design.  Arguments as ``synthesize``."""
    return PulseMaps(*pulse_maps_tensor(field, times, spectrum, wavelengths, weights).unbind(1))
