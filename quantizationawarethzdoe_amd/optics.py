"""Device entry points of the optical elements and the QAT loss (thz_optics.hip).

Gaussian source, thin lens, aperture, the fused |E|^2 -> normalize -> MSE loss, the
polarization analysis of a vectorial field (Stokes vector, ellipse parameters) and the detector
noise models (thz_noise.hip: add_noise, detect), each a
single HIP launch (the loss: two forward, one backward) with torch.autograd glue where a
gradient flows; the image losses of utils/losses.py (thz_losses.hip: dice_loss,
bce_with_logits, ssim, hierarchy_loss); the height-map helpers (thz_heightmap.hip: lut_quantize,
center_difference, total_variation); and the measurement kernels behind utils/metrics.py (thz_metrics.hip:
region_stats, line_widths).  Physical scalars reach the kernels as fp32 host values computed in the
reference's op order; nothing here has a CPU path.
"""
from __future__ import annotations

import collections
import ctypes
import math
import warnings

import numpy as np
import torch

from . import _lib
from .propagation import _require_device, _stream_handle


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _fptr(arr):
    return ctypes.cast(arr, ctypes.POINTER(ctypes.c_float))


def gaussian_beam(H, W, dx, dy, wavelengths, waist_x, waist_y, center=(0.0, 0.0), z_w0=(0.0, 0.0), alpha=0.0,
                  device=None):
    """E [1, C, H, W] complex64 of LightSource/Gaussian_beam.py:88-160 generated on the device."""
    device = torch.device(device) if device is not None else torch.device("cuda")
    if device.type != "cuda":
        raise RuntimeError("gaussian_beam: the MI355X path needs a ROCm device; this framework has no CPU compute path")
    C = len(wavelengths)
    wl, wx, wy = _lib.float_array(wavelengths), _lib.float_array(waist_x), _lib.float_array(waist_y)
    d = _lib.GaussDesc(C=C, H=int(H), W=int(W), dx=float(dx), dy=float(dy), wavelengths=_fptr(wl),
                       waist_x=_fptr(wx), waist_y=_fptr(wy), x0=float(center[0]), y0=float(center[1]),
                       z_w0x=float(z_w0[0]), z_w0y=float(z_w0[1]), alpha=float(alpha))
    out = torch.empty((1, C, int(H), int(W)), dtype=torch.complex64, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().thz_gaussian_beam(ctypes.byref(d), _p(out), _stream_handle()))
    return out


class _Lens(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dx, dy, f, wavelengths):
        _require_device(x, "thin lens")
        x = x.contiguous()
        out = torch.empty_like(x)
        _lens_launch(x, out, dx, dy, f, wavelengths)
        ctx.cfg = (dx, dy, f, wavelengths)
        return out

    @staticmethod
    def backward(ctx, g):
        dx, dy, f, wavelengths = ctx.cfg
        g = g.contiguous()
        out = torch.empty_like(g)
        _lens_launch(g, out, dx, dy, -f, wavelengths)  # conj(ker): the focal length flips sign
        return out, None, None, None, None


def _lens_launch(x, out, dx, dy, f, wavelengths):
    B, C, H, W = x.shape
    wl = _lib.float_array(wavelengths)
    d = _lib.LensDesc(B=B, C=C, H=H, W=W, dx=float(dx), dy=float(dy), focal_length=float(f), wavelengths=_fptr(wl))
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().thz_thin_lens(ctypes.byref(d), _p(x), _p(out), _stream_handle()))


def thin_lens(x, dx, dy, focal_length, wavelengths):
    """field * exp(-i pi r^2 / (lambda f)) (Components/Thin_Lens.py:31-85), differentiable."""
    if x.dtype != torch.complex64:
        raise TypeError(f"lens kernel computes in complex64; got {x.dtype}")
    return _Lens.apply(x, float(dx), float(dy), float(focal_length), tuple(float(w) for w in wavelengths))


class _Aperture(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cfg):
        _require_device(x, "aperture")
        x = x.contiguous()
        out = torch.empty_like(x)
        _aperture_launch(x, out, cfg)
        ctx.cfg = cfg
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        out = torch.empty_like(g)
        _aperture_launch(g, out, ctx.cfg)  # real 0/1 mask: self-adjoint
        return out, None


def _aperture_launch(x, out, cfg):
    kind, dx, dy, half_w, half_h, radius = cfg
    B, C, H, W = x.shape
    d = _lib.ApertureDesc(BC=B * C, H=H, W=W, kind=kind, dx=dx, dy=dy, half_w=half_w, half_h=half_h, radius=radius)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().thz_aperture(ctypes.byref(d), _p(x), _p(out), _stream_handle()))


def aperture(x, kind, dx, dy, half_w=0.0, half_h=0.0, radius=0.0):
    """field * mask (Components/Aperture.py:44-136); thresholds are fp32 as the reference compares them."""
    if x.dtype != torch.complex64:
        raise TypeError(f"aperture kernel computes in complex64; got {x.dtype}")
    cfg = (int(kind), float(dx), float(dy), float(np.float32(half_w)), float(np.float32(half_h)),
           float(np.float32(radius)))
    return _Aperture.apply(x, cfg)


class _IntensityMSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, field, target):
        _require_device(field, "intensity MSE")
        field = field.contiguous()
        target = target.contiguous().float()
        B, C, H, W = field.shape
        t4 = target.reshape((1,) * (4 - target.dim()) + tuple(target.shape))
        d = _lib.LossDesc(B=B, C=C, H=H, W=W, tB=t4.shape[0], tC=t4.shape[1])
        if tuple(t4.shape[-2:]) != (H, W):
            raise ValueError(f"target {tuple(target.shape)} does not broadcast to field {tuple(field.shape)}")
        nbytes = _lib.lib().thz_intensity_mse_workspace_size(ctypes.byref(d))
        stats = torch.empty(nbytes // 4, dtype=torch.float32, device=field.device)
        loss = torch.empty((), dtype=torch.float32, device=field.device)
        with torch.cuda.device(field.device):
            _lib.check(_lib.lib().thz_intensity_mse_forward(ctypes.byref(d), _p(field), _p(t4), _p(loss), _p(stats),
                                                            _stream_handle()))
        ctx.save_for_backward(field, t4, stats)
        ctx.desc = (B, C, H, W, t4.shape[0], t4.shape[1])
        return loss

    @staticmethod
    def backward(ctx, g):
        field, t4, stats = ctx.saved_tensors
        B, C, H, W, tB, tC = ctx.desc
        d = _lib.LossDesc(B=B, C=C, H=H, W=W, tB=tB, tC=tC)
        gf = torch.empty_like(field)
        g = g.detach().float().contiguous()
        with torch.cuda.device(field.device):
            _lib.check(_lib.lib().thz_intensity_mse_backward(ctypes.byref(d), _p(field), _p(t4), _p(stats), _p(g),
                                                             _p(gf), _stream_handle()))
        return gf, None


def intensity_mse(field, target):
    """mean((normalize(|E|^2) - target)^2): the QAT loss of experiment_four_focal_spots.ipynb:336-370
    (normalize = utils/Helper_Functions.py:185-193, per batch item by its max), fused on the device."""
    if field.dtype != torch.complex64:
        raise TypeError(f"loss kernel computes in complex64 fields; got {field.dtype}")
    return _IntensityMSE.apply(field, target)


def field_intensity_mse(field, target):
    """intensity_mse of an ElectricField.  When the field is the deferred output of an ASM_prop
    (propagation.deferred_output), the loss is folded into that propagation's row-inverse pass
    (thz_asm_forward_loss) and the field's data is set from the same pipeline; otherwise this is
    intensity_mse(field.data, target)."""
    pend = field._take_pending_propagation()
    if pend is not None:
        data, loss = pend.run_loss(target)
        field.data = data
        return loss
    return intensity_mse(field.data, target)


class _Resample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, Hout, Wout, dx_in, dy_in, dx_out, dy_out):
        _require_device(x, "field resampler")
        x = x.contiguous()
        B, C, H, W = x.shape
        d = _lib.ResampleDesc(BC=B * C, Hin=H, Win=W, Hout=Hout, Wout=Wout, dx_in=dx_in, dy_in=dy_in, dx_out=dx_out,
                              dy_out=dy_out)
        out = torch.empty((B, C, Hout, Wout), dtype=x.dtype, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().thz_resample_forward(ctypes.byref(d), _p(x), _p(out), _stream_handle()))
        ctx.cfg = (d, (B, C, H, W))
        return out

    @staticmethod
    def backward(ctx, g):
        d, shape = ctx.cfg
        g = g.contiguous()
        gin = torch.empty(shape, dtype=g.dtype, device=g.device)
        with torch.cuda.device(g.device):
            _lib.check(_lib.lib().thz_resample_backward(ctypes.byref(d), _p(g), _p(gin), _stream_handle()))
        return gin, None, None, None, None, None, None


def resample(x, Hout, Wout, dx_in, dy_in, dx_out, dy_out):
    """Bilinear resampling of [B, C, H, W] complex64 onto the centred (Hout, Wout) grid with the
    output pixel pitch (Addons/Field_Resampler.py:74-118), differentiable."""
    if x.dtype != torch.complex64:
        raise TypeError(f"resampler kernel computes in complex64; got {x.dtype}")
    H, W = x.shape[-2:]
    if (H - 1) // 2 == 0 or (W - 1) // 2 == 0:
        # fewer than 3 pixels on an axis: the reference normalises the sampling grid by
        # dx ((H - 1) // 2) = 0 and grid_sample returns NaN everywhere (run here on 1 x 4, 2 x 2 and
        # 2 x 5 fields); the same NaN field, still attached to the input for autograd
        out = torch.full((*x.shape[:-2], int(Hout), int(Wout)), complex(float("nan"), float("nan")),
                         dtype=x.dtype, device=x.device)
        return out + 0 * x.sum(dim=(-2, -1), keepdim=True) if x.requires_grad else out
    return _Resample.apply(x, int(Hout), int(Wout), float(dx_in), float(dy_in), float(dx_out), float(dy_out))


# -------------------------------------------------------------------------------------------------
# Polarization analysis of a vectorial field (Addons/Polarization.py:45-92)
# -------------------------------------------------------------------------------------------------
POLARIZATION_EPS = 1e-6  # Addons/Polarization.py:17


def _check_vector_field(data, comp_dim, who):
    if not torch.is_tensor(data) or not data.is_complex():
        raise TypeError(f"{who}: the field must be a complex tensor")
    if data.dim() < 1 or data.shape[comp_dim] < 2:
        raise ValueError(f"{who}: needs Ex and Ey along dim {comp_dim}; got shape {tuple(data.shape)}")
    _require_device(data, who)
    if data.dtype not in (torch.complex64, torch.complex128):
        raise TypeError(f"{who}: kernels compute in complex64 / complex128; got {data.dtype}")


def _xy_planes(data, comp_dim):
    """The Ex and Ey planes (indices 0 and 1 along ``comp_dim``), each contiguous: views of a
    contiguous [B, ...] tensor with comp_dim = 0, per-component copies otherwise.  A third
    component is never touched."""
    return data.select(comp_dim, 0).contiguous(), data.select(comp_dim, 1).contiguous()


def _pol_launch(entry, ex, ey, *rest):
    with torch.cuda.device(ex.device):
        _lib.check(entry(_p(ex), _p(ey), ex.numel(), *[_p(t) for t in rest], _stream_handle()))


def _four_planes(entry32, entry64, ex, ey):
    """[4, *ex.shape] real planes of one fused entry (one allocation), in the field's precision."""
    wide = ex.dtype == torch.complex128
    out = torch.empty((4, *ex.shape), dtype=torch.float64 if wide else torch.float32, device=ex.device)
    _pol_launch(getattr(_lib.lib(), entry64 if wide else entry32), ex, ey, out)
    return out


class _Stokes(torch.autograd.Function):
    @staticmethod
    def forward(ctx, data, comp_dim):
        ex, ey = _xy_planes(data, comp_dim)
        ctx.save_for_backward(ex, ey)
        ctx.cfg = (comp_dim, tuple(data.shape))
        return _four_planes("thz_stokes_forward", None, ex, ey)

    @staticmethod
    def backward(ctx, g):
        ex, ey = ctx.saved_tensors
        comp_dim, shape = ctx.cfg
        g = g.contiguous().float()
        gd = torch.empty(shape, dtype=ex.dtype, device=ex.device)
        gd.narrow(comp_dim, 2, shape[comp_dim] - 2).zero_()  # Ez (and anything past it) has no part in it
        gx, gy = gd.select(comp_dim, 0), gd.select(comp_dim, 1)
        direct = gx.is_contiguous() and gy.is_contiguous()
        ox, oy = (gx, gy) if direct else (torch.empty_like(ex), torch.empty_like(ey))
        _pol_launch(_lib.lib().thz_stokes_backward, ex, ey, g, ox, oy)
        if not direct:
            gx.copy_(ox)
            gy.copy_(oy)
        return gd, None


def _stokes_torch(data, comp_dim):
    """The Stokes vector from torch ops (differentiable in any precision)."""
    ex, ey = data.select(comp_dim, 0), data.select(comp_dim, 1)
    xx, yy, c = ex.abs() ** 2, ey.abs() ** 2, ex * ey.conj()
    return torch.stack((xx + yy, xx - yy, 2 * c.real, 2 * c.imag))


def stokes(data, comp_dim=0):
    """Stokes vector [4, ...] = (I, Q, U, V) of a complex field whose indices 0 and 1 along
    ``comp_dim`` are Ex and Ey (PolarizationAnalyser.polarization_state, Addons/Polarization.py:
    45-65): I = |Ex|^2 + |Ey|^2, Q = |Ex|^2 - |Ey|^2, U = 2 Re(Ex conj Ey), V = 2 Im(Ex conj Ey), one
    fused pass (thz_stokes_forward).  complex64 is differentiable through thz_stokes_backward;
    complex128 runs thz_stokes64_forward, or torch ops when it requires grad."""
    _check_vector_field(data, comp_dim, "stokes")
    if data.dtype == torch.complex64:
        return _Stokes.apply(data, comp_dim % data.dim())
    if torch.is_grad_enabled() and data.requires_grad:
        return _stokes_torch(data, comp_dim)
    return _four_planes(None, "thz_stokes64_forward", *_xy_planes(data, comp_dim))


def polarization_ellipse(data, comp_dim=0):
    """Ellipse parameters [4, ...] = (A, B, theta, h) (PolarizationAnalyser.polarization_ellipse,
    Addons/Polarization.py:67-92, eps = 1e-6): Ip = sqrt(Q^2 + U^2 + V^2), L = (Q + eps) + i U,
    A = sqrt((Ip + |L| + eps) / 2), B = sqrt((Ip - |L| + eps) / 2), theta = atan2(U, Q + eps) / 2,
    h = sign(V + eps).  One fused pass from the fields (thz_polarization_ellipse) when no gradient
    is wanted; under autograd the same sequence in torch ops on the differentiable ``stokes``.

    Deviation from the reference: B's radicand is clamped at 0.  On exactly linear polarization
    rounding leaves it slightly negative and the reference returns NaN there (Ey = 0.5 Ex in fp32:
    2 of 480 pixels)."""
    _check_vector_field(data, comp_dim, "polarization_ellipse")
    if not (torch.is_grad_enabled() and data.requires_grad):
        return _four_planes("thz_polarization_ellipse", "thz_polarization_ellipse64", *_xy_planes(data, comp_dim))
    _, Q, U, V = stokes(data, comp_dim)
    eps = POLARIZATION_EPS
    Ip = torch.sqrt(Q ** 2 + U ** 2 + V ** 2)
    Lr = Q + eps
    aL = torch.hypot(Lr, U)
    A = torch.sqrt(0.5 * (Ip + aL + eps))
    B = torch.sqrt(torch.clamp(0.5 * (Ip - aL + eps), min=0))
    return torch.stack((A, B, 0.5 * torch.atan2(U, Lr), torch.sign(V + eps)))


# -------------------------------------------------------------------------------------------------
# Detector noise models (Addons/Noise.py, utils/Noise.py, utils/Helper_Functions.py:258-366)
# -------------------------------------------------------------------------------------------------
NOISE_KINDS = {"gauss": _lib.NOISE_GAUSS, "uniform": _lib.NOISE_UNIFORM, "poisson": _lib.NOISE_POISSON,
               "poisson_gauss": _lib.NOISE_POISSON_GAUSS}


def _noise_kind(kind):
    try:
        return NOISE_KINDS[str(kind).lower()]
    except KeyError:
        raise ValueError(f"noise kind must be one of {sorted(NOISE_KINDS)}; got {kind!r}") from None


def _noise_state(x, rng):
    """(state, stream) of a call: the caller's pair, or a state drawn on the device from torch's
    generator (no sync; torch.manual_seed reproduces it) with stream 0."""
    if rng is None:
        return torch.randint(0, 2 ** 31 - 1, (2,), dtype=torch.int32, device=x.device), 0
    state, stream = rng
    if not torch.is_tensor(state) or state.dtype != torch.int32 or state.numel() != 2 or state.device != x.device:
        raise TypeError("rng = (state, stream): state must be an int32 [2] tensor (seed, step) on the input's device")
    return state, int(stream)


def _noise_apply(kind, inp, x, out, state, stream, sigma, a, gain, normalize, sigma_dev=None):
    d = _lib.NoiseDesc(kind=kind, input=inp, sigma=float(sigma), a=float(a), gain=float(gain),
                       normalize=int(bool(normalize)), sigma_dev=sigma_dev.data_ptr() if sigma_dev is not None else None,
                       rng=state.data_ptr(), stream=stream)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().thz_noise_apply(ctypes.byref(d), _p(x), _p(out), x.numel(), _stream_handle()))


def _sum_workspace(x):
    nbytes = ctypes.c_size_t(0)
    _lib.check(_lib.lib().thz_signal_scale_workspace_size(x.numel(), ctypes.byref(nbytes)))
    return torch.empty(nbytes.value, dtype=torch.uint8, device=x.device)


def signal_scale(x, snr_linear):
    """sqrt(mean(|x|^2) / snr_linear) of a float32 / complex64 device tensor as a device scalar [1]
    (utils/Noise.py:28-32): summed in fp64 in a fixed order, rounded to fp32 once, no sync
    (thz_signal_scale)."""
    _require_device(x, "signal_scale")
    x = x.contiguous()
    scale = torch.empty(1, dtype=torch.float32, device=x.device)
    ws = _sum_workspace(x)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().thz_signal_scale(_p(x), x.numel(), int(x.is_complex()), float(snr_linear), _p(scale),
                                               _p(ws), ws.numel(), _stream_handle()))
    return scale


def noise_draws(what, rng, n, device=None):
    """The raw draws of elements 0 .. n-1 of rng = (state, stream) that the noise kernels use
    (thz_noise_draws): what = "normal" [n], "uniform" [n] or "complex_normal" [n] complex64."""
    state, stream = rng
    code = {"normal": _lib.DRAW_NORMAL, "uniform": _lib.DRAW_UNIFORM, "complex_normal": _lib.DRAW_COMPLEX_NORMAL}[what]
    _require_device(state, "noise_draws")
    out = torch.empty(2 * n if what == "complex_normal" else n, dtype=torch.float32, device=state.device)
    with torch.cuda.device(state.device):
        _lib.check(_lib.lib().thz_noise_draws(code, _p(state), int(stream), int(n), _p(out), _stream_handle()))
    return torch.view_as_complex(out.view(n, 2)) if what == "complex_normal" else out


class _Noise(torch.autograd.Function):
    """y = model(x) (inp REAL32 / COMPLEX64) or model(|x|^2) (inp FIELD_INTENSITY).  cfg = (kind, inp,
    sigma, a, gain, normalize, snr_linear)."""

    @staticmethod
    def forward(ctx, x, state, stream, cfg):
        kind, inp, sigma, a, gain, normalize, snr = cfg
        x = x.contiguous()
        real_out = inp != _lib.NOISE_IN_COMPLEX64
        out = torch.empty(x.shape, dtype=torch.float32 if real_out else torch.complex64, device=x.device)
        scale = signal_scale(x, snr) if snr is not None else None
        _noise_apply(kind, inp, x, out, state, stream, sigma, a, gain, normalize, scale)
        ctx.cfg = (kind, inp, snr, stream)
        ctx.save_for_backward(x, state, *(() if scale is None else (scale,)))
        return out

    @staticmethod
    def backward(ctx, g):
        kind, inp, snr, stream = ctx.cfg
        x, state, *scale = ctx.saved_tensors
        if kind in (_lib.NOISE_POISSON, _lib.NOISE_POISSON_GAUSS):
            return torch.zeros_like(x), None, None, None  # torch's derivative of poisson()
        g = g.contiguous()
        if snr is not None:  # y = x + n scale(x): the scale depends on every element
            gx = torch.empty_like(x)
            ws = _sum_workspace(x)
            with torch.cuda.device(x.device):
                _lib.check(_lib.lib().thz_snr_noise_backward(
                    _p(g), _p(x), x.numel(), int(x.is_complex()), float(snr), _p(scale[0]), _p(state), stream,
                    _p(gx), _p(ws), ws.numel(), _stream_handle()))
            return gx, None, None, None
        if inp == _lib.NOISE_IN_FIELD_INTENSITY:
            return 2 * g * x, None, None, None  # d|E|^2: 2 g E in torch's convention
        return g, None, None, None


def _noise_torch(x, kind, sigma, a, gain, normalize, snr):
    """The reference's torch op sequence (Addons/Noise.py:27, 58-61, 87-89, 112, utils/Noise.py:28-32)
    for the precisions the kernels do not compute in; draws from torch's generator."""
    if snr is not None:
        return x + torch.randn_like(x) * torch.sqrt(torch.mean(x.abs() ** 2) / snr)
    if kind == _lib.NOISE_GAUSS:
        return x + torch.randn_like(x) * sigma
    if kind == _lib.NOISE_UNIFORM:
        return x + (torch.rand_like(x) - 0.5) * 2 * a
    y = torch.poisson(x / gain)
    if kind == _lib.NOISE_POISSON:
        return y * gain if normalize else y
    return y * gain + torch.randn_like(x) * sigma


def _noise_cfg(kind, sigma, a, gain, normalize, snr_db, who):
    k = _noise_kind(kind)
    snr = None
    if snr_db is not None:
        if k != _lib.NOISE_GAUSS:
            raise ValueError(f"{who}: snr_db scales Gaussian noise; got kind {kind!r}")
        snr = 10 ** (float(snr_db) / 10)  # utils/Noise.py:29
    return k, float(sigma), float(a), float(gain), bool(normalize), snr


def add_noise(x, kind, *, sigma=0.1, a=0.1, gain=1.0, normalize=True, snr_db=None, rng=None):
    """A detector noise model applied to a measurement ``x`` in one fused pass (thz_noise_apply).

    kind: "gauss"  x + n sigma (Addons/Noise.py:27), or with ``snr_db`` x + n sqrt(mean(|x|^2) / 10^(snr_db / 10))
    (utils/Noise.py:28-32; real or complex x, the scale a device scalar from thz_signal_scale);
    "uniform"  x + (u - 0.5) 2 a; "poisson"  poisson(x / gain), times gain if ``normalize``;
    "poisson_gauss"  poisson(x / gain) gain + n sigma.

    rng = (state, stream): the int32 [2] device tensor (seed, step) and stream of ``doe.modulate`` --
    the same pair gives the same sample, a captured graph draws afresh once the host advances
    state[1].  Streams are independent of each other under one seed (use one state and number the
    streams, as the trainers do): the generator folds the stream into the seed word, so unrelated
    (seed, stream) pairs can coincide.  rng = None draws the state from torch's generator on the
    device per call (torch.manual_seed reproduces a run; nothing syncs).

    Gradients as in the reference: "gauss" and "uniform" pass the gradient through, the SNR form
    adds the scale's dependence on x (thz_snr_noise_backward), and the Poisson kinds return zeros --
    torch's derivative of ``poisson``.  float64 / complex128 device tensors run the reference's torch
    op sequence on torch's generator instead (``rng`` is not used)."""
    cfg = _noise_cfg(kind, sigma, a, gain, normalize, snr_db, "add_noise")
    if not torch.is_tensor(x) or not (x.is_floating_point() or x.is_complex()):
        raise TypeError("add_noise: x must be a floating-point or complex tensor")
    if x.is_complex() and cfg[0] != _lib.NOISE_GAUSS:
        raise TypeError(f"add_noise: {kind!r} noise is defined for real measurements only (the reference's "
                        "rand_like - 0.5 on a complex tensor shifts the real part alone); got " + str(x.dtype))
    _require_device(x, "add_noise")
    if x.dtype in (torch.float64, torch.complex128):
        return _noise_torch(x, *cfg)
    if x.dtype not in (torch.float32, torch.complex64):
        raise TypeError(f"add_noise: kernels compute in float32 / complex64; got {x.dtype}")
    state, stream = _noise_state(x, rng)
    inp = _lib.NOISE_IN_COMPLEX64 if x.is_complex() else _lib.NOISE_IN_REAL32
    return _Noise.apply(x, state, stream, (cfg[0], inp) + cfg[1:])


def detect(field, kind, *, sigma=0.1, a=0.1, gain=1.0, normalize=True, rng=None):
    """The noisy intensity measurement of a complex field (tensor or ElectricField) in one pass:
    ``add_noise(field.abs() ** 2, kind, ...)`` without materialising the intensity -- 8 B read and
    4 B written per pixel.  The gradient chains the intensity's 2 g E ("gauss", "uniform") or is
    zero (the Poisson kinds).  complex128 fields run the reference's torch op sequence."""
    data = field if torch.is_tensor(field) else getattr(field, "data", field)
    cfg = _noise_cfg(kind, sigma, a, gain, normalize, None, "detect")
    if not torch.is_tensor(data) or not data.is_complex():
        raise TypeError("detect: the field must be a complex tensor or an ElectricField")
    _require_device(data, "detect")
    if data.dtype == torch.complex128:
        return _noise_torch(data.abs() ** 2, *cfg)
    if data.dtype != torch.complex64:
        raise TypeError(f"detect: kernels compute in complex64; got {data.dtype}")
    state, stream = _noise_state(data, rng)
    return _Noise.apply(data, state, stream, (cfg[0], _lib.NOISE_IN_FIELD_INTENSITY) + cfg[1:])


# -------------------------------------------------------------------------------------------------
# Fabrication-tolerance screen (thz_tolerance.hip) behind tolerance.py
# -------------------------------------------------------------------------------------------------
TOLERANCE_ROUGHNESS = {"uniform": _lib.TOL_ROUGH_UNIFORM, "normal": _lib.TOL_ROUGH_NORMAL}


def _tolerance_cfg(fab, who):
    """(sigma_scale, level table, roughness code, roughness, lo, hi) of a ``tolerance.FabricationModel`` (or
    anything with its four attributes); a scalar ``sigma_level`` other than 0 serves every level index."""
    levels = fab.sigma_level
    if isinstance(levels, (int, float)):
        levels = (float(levels),) * _lib.THZ_MAX_LUT if float(levels) != 0.0 else ()
    levels = tuple(float(v) for v in levels)
    if len(levels) > _lib.THZ_MAX_LUT:
        raise ValueError(f"{who}: {len(levels)} level sigmas; the kernel takes up to {_lib.THZ_MAX_LUT}")
    code, rough = _lib.TOL_ROUGH_NONE, 0.0
    if fab.roughness is not None:
        name, rough = fab.roughness
        if name not in TOLERANCE_ROUGHNESS:
            raise ValueError(f"{who}: roughness must be None, ('uniform', a) or ('normal', s); got {fab.roughness!r}")
        code, rough = TOLERANCE_ROUGHNESS[name], float(rough)
    lo, hi = fab.clamp
    return (float(fab.sigma_scale), levels, code, rough, -math.inf if lo is None else float(lo),
            math.inf if hi is None else float(hi))


def _tolerance_desc(cfg, K, first, field, height, eps, tand, wavelengths, state, stream):
    sigma_scale, levels, code, rough, lo, hi = cfg
    Bf, C, H, W = field.shape
    wl = _lib.float_array(wavelengths)
    d = _lib.ToleranceDesc(K=K, first=first, Bf=Bf, C=C, H=H, W=W, hs=height.shape[0], ws=height.shape[1],
                           L=len(levels), sigma_level=(ctypes.c_float * _lib.THZ_MAX_LUT)(*levels),
                           sigma_scale=sigma_scale, rough_kind=code, rough=rough, lo=lo, hi=hi,
                           epsilon=eps, tand=tand, wavelengths=_fptr(wl), rng=state.data_ptr(), stream=stream)
    d._keep = wl
    return d


class _ToleranceModulate(torch.autograd.Function):
    """out [K, C, H, W] (and the realised maps [K, hs, ws]) of thz_tolerance_modulate_forward.  args = (K, first,
    stream, eps, tand, wavelengths, cfg, want_heights)."""

    @staticmethod
    def forward(ctx, field, height, idx, state, args):
        K, first, stream, eps, tand, wavelengths, cfg, want_heights = args
        field, height = field.contiguous(), height.detach().contiguous()
        d = _tolerance_desc(cfg, K, first, field, height, eps, tand, wavelengths, state, stream)
        out = torch.empty((K,) + tuple(field.shape[1:]), dtype=torch.complex64, device=field.device)
        heights = torch.empty((K,) + tuple(height.shape), dtype=torch.float32, device=field.device) if want_heights else None
        with torch.cuda.device(field.device):
            _lib.check(_lib.lib().thz_tolerance_modulate_forward(ctypes.byref(d), _p(field), _p(height), _p(idx), _p(out),
                                                                 _p(heights), _stream_handle()))
        ctx.save_for_backward(field, height, idx, state)
        ctx.args = args
        if heights is not None:
            ctx.mark_non_differentiable(heights)
        return out, heights

    @staticmethod
    def backward(ctx, g, _gh):
        field, height, idx, state = ctx.saved_tensors
        K, first, stream, eps, tand, wavelengths, cfg, _ = ctx.args
        d = _tolerance_desc(cfg, K, first, field, height, eps, tand, wavelengths, state, stream)
        g = g.contiguous()
        gf = torch.empty_like(field) if ctx.needs_input_grad[0] else None
        gh = torch.empty_like(height) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(field.device):
            _lib.check(_lib.lib().thz_tolerance_modulate_backward(ctypes.byref(d), _p(g), _p(field), _p(height), _p(idx),
                                                                  _p(gf), _p(gh), None, 0, _stream_handle()))
        return gf, gh, None, None, None


def tolerance_modulate(field, height, wavelengths, eps, tand, fab, K, *, idx=None, rng=None, first=0,
                       return_heights=False):
    """K fabrication-perturbed realisations of the height map ``height`` applied to ``field`` in one streaming
    pass (thz_tolerance_modulate_forward): ``out[k] = field[b] * t(h_k)`` with, for realisation ``first + k``,

        h_k = clamp((1 + g_k) h + e_{k, idx} + r_k, lo, hi)

    -- a depth-scale error g_k = sigma_scale n, a depth error per level e_{k,l} = sigma_level[l] n (``idx`` [hs,
    ws] gives every map pixel's level, e.g. from ``lut_quantize(h, lut, mode="argmin")``; a value outside the
    table takes none) and a per-pixel roughness r_k (the reference's ``(u - 0.5) 2 a`` or ``s n``), as
    ``fab``, a ``tolerance.FabricationModel``, states them.

    ``field``: complex64 [1, C, H, W] (one incident field for every realisation) or [K, C, H, W]; ``height``:
    float32 [hs, ws], upsampled to the field by the nearest rule of ``doe.modulate``.  Returns ``out`` [K, C, H,
    W], and ``(out, heights)`` with the realised maps [K, hs, ws] when ``return_heights``; ``out[k]`` equals
    ``doe.modulate(field, heights[k])`` bit for bit.

    ``rng = (state, stream)`` as in ``add_noise`` (None: a state drawn on the device from torch's generator).
    Realisation k is a pure function of (state, stream, k): chunks of a run (``first`` advancing) give the bits
    of one call.  Gradients flow to ``height`` and ``field`` (thz_tolerance_modulate_backward: every draw
    regenerated, fp64 sums in a fixed order, no atomics), which makes the mean of a loss over the K outputs
    a robust-design objective.  No host sync; capturable in torch.cuda.graph."""
    who = "tolerance_modulate"
    if not torch.is_tensor(field) or not torch.is_tensor(height):
        raise TypeError(f"{who}: field and height must be tensors")
    _require_device(field, who)
    _require_device(height, who)
    if field.dtype != torch.complex64 or height.dtype != torch.float32:
        raise TypeError(f"{who}: the kernel computes in complex64 / float32; got {field.dtype} and {height.dtype}")
    K, first = int(K), int(first)
    if K < 1 or first < 0:
        raise ValueError(f"{who}: K = {K} must be >= 1 and first = {first} >= 0")
    if field.dim() != 4 or field.shape[0] not in (1, K):
        raise ValueError(f"{who}: the field must be [1, C, H, W] or [K = {K}, C, H, W]; got {tuple(field.shape)}")
    if height.dim() != 2:
        raise ValueError(f"{who}: one height map [hs, ws]; got {tuple(height.shape)}")
    wl = tuple(float(w) for w in wavelengths)
    if len(wl) != field.shape[1]:
        raise ValueError(f"{who}: {len(wl)} wavelengths for a field of {field.shape[1]} channels")
    cfg = _tolerance_cfg(fab, who)
    if idx is not None:
        if not torch.is_tensor(idx) or idx.shape != height.shape or idx.device != height.device:
            raise ValueError(f"{who}: idx must be an integer tensor of the map's shape on its device")
        idx = idx.to(torch.int32).contiguous()
    elif any(v != 0.0 for v in cfg[1]):
        raise ValueError(f"{who}: a per-level error needs idx, the level index of every map pixel")
    state, stream = _noise_state(field, rng)
    out, heights = _ToleranceModulate.apply(field, height, idx, state, (K, first, stream, float(eps), float(tand), wl,
                                                                        cfg, bool(return_heights)))
    return (out, heights) if return_heights else out


# ---- image losses (utils/losses.py on thz_losses.hip) ------------------------------------------
def _loss_pair(pred, target, who):
    """The checks every loss shares; returns the contiguous pair."""
    if not torch.is_tensor(pred) or not torch.is_tensor(target):
        raise TypeError(f"{who}: pred and target must be tensors")
    _require_device(pred, who)
    _require_device(target, who)
    if pred.dtype != torch.float32 or target.dtype != torch.float32:
        raise TypeError(f"{who}: kernels compute in float32; got {pred.dtype} and {target.dtype}")
    if target.requires_grad:
        raise NotImplementedError(f"{who}: the gradient with respect to target is not implemented; detach it")
    if pred.numel() == 0:
        raise ValueError(f"{who}: empty input {tuple(pred.shape)}")
    return pred.contiguous(), target.contiguous()


def _plane_like(w, pred, name):
    """weight / pos_weight expanded to pred's shape (torch broadcasts them; the kernel reads a plane)."""
    if w is None:
        return None
    w = torch.as_tensor(w, dtype=torch.float32, device=pred.device)
    if w.requires_grad:
        raise NotImplementedError(f"bce_with_logits: the gradient with respect to {name} is not implemented")
    return w.expand(pred.shape).contiguous()


def _dice_bce_desc(pred, terms, p=2.0, smooth=1.0, weight=None, pos_weight=None, elementwise=False):
    n = pred.shape[0] if pred.dim() else 1
    return _lib.DiceBceDesc(N=n, M=pred.numel() // n, p=float(p), smooth=float(smooth), terms=terms,
                            bce_grad_elementwise=int(elementwise),
                            weight=weight.data_ptr() if weight is not None else None,
                            pos_weight=pos_weight.data_ptr() if pos_weight is not None else None)


def _dice_bce_sums(pred, target, d, want_map=False):
    """sums [N, 4] float64 (sum p t, sum p^e, sum t^e, sum bce) and the BCE map or None."""
    sums = torch.empty((d.N, 4), dtype=torch.float64, device=pred.device)
    bmap = torch.empty_like(pred) if want_map else None
    nbytes = ctypes.c_size_t(0)
    _lib.check(_lib.lib().thz_dice_bce_sums_workspace_size(ctypes.byref(d), ctypes.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=pred.device)
    with torch.cuda.device(pred.device):
        _lib.check(_lib.lib().thz_dice_bce_sums(ctypes.byref(d), _p(pred), _p(target), _p(sums), _p(bmap), _p(ws),
                                                ws.numel(), _stream_handle()))
    return sums, bmap


def _dice_bce_backward(pred, target, d, sums, g_dice, g_bce):
    grad = torch.empty_like(pred)
    with torch.cuda.device(pred.device):
        _lib.check(_lib.lib().thz_dice_bce_backward(ctypes.byref(d), _p(pred), _p(target), _p(sums), _p(g_dice),
                                                    _p(g_bce), _p(grad), _stream_handle()))
    return grad


def _dice_from_sums(sums, smooth):
    """1 - num / den per sample (utils/losses.py:32-35) on the fp64 sums."""
    return 1 - (sums[:, 0] + smooth) / (sums[:, 1] + sums[:, 2] + smooth)


class _Dice(torch.autograd.Function):
    """The per-sample Dice loss [N] of contiguous pred, target."""

    @staticmethod
    def forward(ctx, pred, target, smooth, p):
        sums, _ = _dice_bce_sums(pred, target, _dice_bce_desc(pred, _lib.LOSS_TERM_DICE, p, smooth))
        ctx.save_for_backward(pred, target, sums)
        ctx.cfg = (smooth, p)
        return _dice_from_sums(sums, smooth).float()

    @staticmethod
    def backward(ctx, g):
        pred, target, sums = ctx.saved_tensors
        smooth, p = ctx.cfg
        d = _dice_bce_desc(pred, _lib.LOSS_TERM_DICE, p, smooth)
        return _dice_bce_backward(pred, target, d, sums, g.float().contiguous(), None), None, None, None


class _Bce(torch.autograd.Function):
    """BCE with logits of contiguous pred, target: the map (reduction 'none') or the sum times ``scale``."""

    @staticmethod
    def forward(ctx, pred, target, weight, pos_weight, reduction):
        none = reduction == "none"
        d = _dice_bce_desc(pred, _lib.LOSS_TERM_BCE, weight=weight, pos_weight=pos_weight)
        sums, bmap = _dice_bce_sums(pred, target, d, want_map=none)
        ctx.save_for_backward(pred, target, *(w for w in (weight, pos_weight) if w is not None))
        ctx.cfg = (weight is not None, pos_weight is not None, none,
                   1.0 / pred.numel() if reduction == "mean" else 1.0)
        return bmap if none else (sums[:, 3].sum() * ctx.cfg[3]).float()

    @staticmethod
    def backward(ctx, g):
        has_w, has_pw, none, scale = ctx.cfg
        pred, target, *planes = ctx.saved_tensors
        weight = planes.pop(0) if has_w else None
        pos_weight = planes.pop(0) if has_pw else None
        d = _dice_bce_desc(pred, _lib.LOSS_TERM_BCE, weight=weight, pos_weight=pos_weight, elementwise=none)
        g = g.float().contiguous() if none else (g.float() * scale).reshape(1)
        return _dice_bce_backward(pred, target, d, None, None, g), None, None, None, None


def _reduce(loss, reduction):
    if reduction == "mean":
        return loss.mean()
    if reduction == "sum":
        return loss.sum()
    if reduction == "none":
        return loss
    raise Exception("Unexpected reduction {}".format(reduction))


def dice_loss(pred, target, smooth=1, p=2, reduction="mean"):
    """BinaryDiceLoss (utils/losses.py:7-44): 1 - (sum p t + smooth) / (sum p^e + sum t^e + smooth) per
    sample of [N, *] inputs, then ``reduction``; one streaming pass forward (thz_dice_bce_sums), one
    backward (thz_dice_bce_backward), differentiable in ``pred``."""
    if reduction not in ("mean", "sum", "none"):
        raise Exception("Unexpected reduction {}".format(reduction))
    pred, target = _loss_pair(pred, target, "dice_loss")
    assert pred.shape[0] == target.shape[0], "predict & target batch size don't match"
    if pred.numel() != target.numel():
        raise ValueError(f"dice_loss: pred {tuple(pred.shape)} and target {tuple(target.shape)} differ in size")
    return _reduce(_Dice.apply(pred, target, float(smooth), float(p)), reduction)


def bce_with_logits(pred, target, weight=None, pos_weight=None, reduction="mean"):
    """torch.nn.BCEWithLogitsLoss (BinaryCEloss, utils/losses.py:47-58) in one streaming pass forward
    and one backward; ``weight`` / ``pos_weight`` broadcast to ``pred``; differentiable in ``pred``."""
    if reduction not in ("mean", "sum", "none"):
        raise ValueError(f"{reduction} is not a valid value for reduction")
    pred, target = _loss_pair(pred, target, "bce_with_logits")
    if pred.shape != target.shape:
        raise ValueError(f"Target size ({target.size()}) must be the same as input size ({pred.size()})")
    return _Bce.apply(pred, target, _plane_like(weight, pred, "weight"), _plane_like(pos_weight, pred, "pos_weight"),
                      reduction)


_ssim_windows = {}


def _ssim_window(win_size, win_sigma):
    """The 1-D Gaussian taps as pytorch_msssim forms them: float32 torch ops on the host."""
    key = (int(win_size), float(win_sigma))
    if key not in _ssim_windows:
        coords = torch.arange(key[0], dtype=torch.float32) - key[0] // 2
        g = torch.exp(-(coords ** 2) / (2 * key[1] ** 2))
        _ssim_windows[key] = tuple((g / g.sum()).tolist())
    return _ssim_windows[key]


def _ssim_desc(x, window, C1, C2, nonnegative=False, accumulate=False):
    N, C, H, W = x.shape
    d = _lib.SsimDesc(NC=N * C, H=H, W=W, ws=len(window), C1=C1, C2=C2, nonnegative=int(nonnegative),
                      accumulate=int(accumulate))
    for i, w in enumerate(window[:_lib.SSIM_MAX_WIN]):
        d.window[i] = w
    return d


def _ssim_forward(x, y, d, want_coef):
    """ssim [N, C] and the backward's coefficient planes [3, N, C, H', W'] or None."""
    N, C, H, W = x.shape
    out = torch.empty((N, C), dtype=torch.float32, device=x.device)
    coef = None
    if want_coef:
        wh, ww = (1 if H < d.ws else d.ws), (1 if W < d.ws else d.ws)
        coef = torch.empty((3, N, C, H - wh + 1, W - ww + 1), dtype=torch.float32, device=x.device)
    nbytes = ctypes.c_size_t(0)
    _lib.check(_lib.lib().thz_ssim_workspace_size(ctypes.byref(d), ctypes.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().thz_ssim_forward(ctypes.byref(d), _p(x), _p(y), _p(out), None, _p(coef), _p(ws),
                                               ws.numel(), _stream_handle()))
    return out, coef


def _ssim_backward(x, y, d, coef, out, g, grad):
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().thz_ssim_backward(ctypes.byref(d), _p(x), _p(y), _p(coef), _p(out), _p(g), _p(grad),
                                                _stream_handle()))
    return grad


class _Ssim(torch.autograd.Function):
    """ssim per (n, c) [N, C] of contiguous x, y [N, C, H, W]; cfg = (window, C1, C2, nonnegative)."""

    @staticmethod
    def forward(ctx, x, y, cfg):
        out, coef = _ssim_forward(x, y, _ssim_desc(x, *cfg), ctx.needs_input_grad[0])
        if coef is not None:
            ctx.save_for_backward(x, y, coef, out)
        ctx.cfg = cfg
        return out

    @staticmethod
    def backward(ctx, g):
        x, y, coef, out = ctx.saved_tensors
        grad = _ssim_backward(x, y, _ssim_desc(x, *ctx.cfg), coef, out, g.float().contiguous(), torch.empty_like(x))
        return grad, None, None


def _ssim_cfg(x, y, win_size, win_sigma, data_range, K, nonnegative_ssim, who):
    if x.shape != y.shape:
        raise ValueError(f"Input images should have the same dimensions, but got {x.shape} and {y.shape}.")
    if x.dim() == 5:
        raise NotImplementedError(f"{who}: 3-D (5-d input) SSIM is not implemented; got {x.shape}")
    if x.dim() != 4:
        raise ValueError(f"Input images should be 4-d or 5-d tensors, but got {x.shape}")
    if int(win_size) % 2 != 1:
        raise ValueError("Window size should be odd.")
    for i, n in enumerate(x.shape[2:]):
        if n < win_size:
            warnings.warn(f"Skipping Gaussian Smoothing at dimension 2+{i} for input: {x.shape} and win size: {win_size}")
    return (_ssim_window(win_size, win_sigma), (float(K[0]) * float(data_range)) ** 2,
            (float(K[1]) * float(data_range)) ** 2, bool(nonnegative_ssim))


def ssim(x, y, *, win_size=11, win_sigma=1.5, data_range=1.0, K=(0.01, 0.03), size_average=True,
         nonnegative_ssim=False):
    """pytorch_msssim.ssim (the measure behind SSIMloss, utils/losses.py:62-74) of [N, C, H, W] images:
    the mean over the valid window positions of the SSIM map, per (n, c), then the mean over all
    (a scalar) or over C ([N], ``size_average=False``).  One tiled kernel reads x and y once
    (thz_ssim_forward) and, when x needs a gradient, writes the three coefficient planes its backward
    gathers from (thz_ssim_backward); differentiable in ``x``."""
    cfg = _ssim_cfg(x, y, win_size, win_sigma, data_range, K, nonnegative_ssim, "ssim")
    x, y = _loss_pair(x, y, "ssim")
    per_channel = _Ssim.apply(x, y, cfg)
    return per_channel.mean() if size_average else per_channel.mean(1)


class _Hierarchy(torch.autograd.Function):
    """bce(pred, t) + dice(pred, t) + 1 - ssim(pred, t) with the references' defaults, all means."""

    @staticmethod
    def forward(ctx, pred, target, cfg):
        both = _lib.LOSS_TERM_DICE | _lib.LOSS_TERM_BCE
        sums, _ = _dice_bce_sums(pred, target, _dice_bce_desc(pred, both))
        out, coef = _ssim_forward(pred, target, _ssim_desc(pred, *cfg), ctx.needs_input_grad[0])
        if coef is not None:
            ctx.save_for_backward(pred, target, sums, coef, out)
        ctx.cfg = cfg
        loss = sums[:, 3].sum() / pred.numel() + _dice_from_sums(sums, 1.0).mean() + (1 - out.double().mean())
        return loss.float()

    @staticmethod
    def backward(ctx, g):
        pred, target, sums, coef, out = ctx.saved_tensors
        N, C = pred.shape[:2]
        g = g.float()
        d = _dice_bce_desc(pred, _lib.LOSS_TERM_DICE | _lib.LOSS_TERM_BCE)
        grad = _dice_bce_backward(pred, target, d, sums, (g / N).expand(N).contiguous(),
                                  (g / pred.numel()).reshape(1))
        gs = (-g / (N * C)).expand(N, C).contiguous()
        _ssim_backward(pred, target, _ssim_desc(pred, *ctx.cfg, accumulate=True), coef, out, gs, grad)
        return grad, None, None


def hierarchy_loss(pred, target):
    """Hierarchyloss (utils/losses.py:78-88): BinaryCEloss + BinaryDiceLoss + SSIMloss at their defaults
    on the same ``pred`` -- as logits for the BCE term and as a probability for Dice and SSIM, the
    reference's own use.  One thz_dice_bce_sums pass serves the Dice and BCE terms; the backward is one
    thz_dice_bce_backward pass plus the SSIM gather adding into the same gradient."""
    cfg = _ssim_cfg(pred, target, 11, 1.5, 1.0, (0.01, 0.03), False, "hierarchy_loss")
    pred, target = _loss_pair(pred, target, "hierarchy_loss")
    return _Hierarchy.apply(pred, target, cfg)


# ---- height-map helpers (thz_heightmap.hip) ----------------------------------------------------
_LUT_MODES = {"bucketize": _lib.LUTQ_BUCKETIZE, "argmin": _lib.LUTQ_ARGMIN}
_LUT_KINDS = {"identity": _lib.LUTQ_GRAD_IDENTITY, "poly": _lib.LUTQ_GRAD_POLY, "sigmoid": _lib.LUTQ_GRAD_SIGMOID}


def _table(values, who, dtype):
    """A table's values in x's precision as a tuple of host floats (they travel by value in the
    descriptor).  A list or a CPU tensor costs nothing on the device.  A device tensor is read back
    (a device-to-host copy that waits for the stream) on every call -- nothing is remembered, since
    neither a tensor's address nor its version pins its values -- and is refused while a graph is
    being captured, where such a read is not allowed."""
    if torch.is_tensor(values):
        t = values.detach().reshape(-1)
        if t.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{who}: a table given as a device tensor must be read back to the host, which a graph "
                               "capture does not allow; pass the table as a list or a CPU tensor")
        return tuple(t.to(dtype).tolist())
    try:
        return tuple(torch.tensor([float(v) for v in values], dtype=torch.float64).to(dtype).tolist())
    except TypeError:
        raise TypeError(f"{who}: the table must be a tensor or a sequence of numbers") from None


def _lut_mid(lut, dtype):
    """lut_mid (utils/Helper_Functions.py:371-372) of the levels, in x's precision."""
    t = torch.tensor(lut, dtype=dtype)
    return tuple(((t[:-1] + t[1:]) / 2).tolist())


def _lut_desc(n, mode, wrap, kind, lut, thr):
    d = _lib.LutQuantizeDesc(n=n, mode=mode, wrap=int(wrap), kind=kind, L=len(lut), T=len(thr))
    for i, v in enumerate(lut[:_lib.THZ_MAX_LUT]):
        d.lut[i] = v
    for i, v in enumerate(thr[:_lib.THZ_MAX_LUT]):
        d.thresholds[i] = v
    return d


def _lut_forward_torch(x, lut, thr, mode, wrap):
    """The reference's op sequence: nearest_idx (utils/Helper_Functions.py:390-398) or the notebooks'
    argmin snap.  Returns (q, idx int64)."""
    lut_t = torch.tensor(lut, dtype=x.dtype, device=x.device)
    if mode == _lib.LUTQ_ARGMIN:
        idx = torch.argmin(torch.abs(x.unsqueeze(-1) - lut_t), dim=-1)
    else:
        idx = torch.bucketize(x, torch.tensor(thr, dtype=x.dtype, device=x.device), right=True)
        if wrap:
            idx = idx % len(thr)
    return lut_t[idx], idx


def _lut_slope_torch(x, idx, lut, kind, s):
    """The surrogate slopes of Components/quantization.py:79-122 as torch ops, with the kernel's index
    rules (sign 0 when x - q is zero or not finite; idx + d taken modulo the number of levels)."""
    lut_t = torch.tensor(lut, dtype=x.dtype, device=x.device)
    q = lut_t[idx]
    dx = x - q
    d = torch.where(torch.isfinite(dx), torch.sign(dx), torch.zeros_like(dx)).long()
    other = lut_t[torch.remainder(idx + d, len(lut))]
    mid = (other + q) / 2
    gap = torch.abs(other - q) + 1e-20
    z = (x - mid) / gap * 2
    if kind == _lib.LUTQ_GRAD_POLY:
        return (0.5 * s * (1 - abs(z)) ** (s - 1)).nan_to_num() * 2.
    z = z * s
    return torch.sigmoid(z) * (1 - torch.sigmoid(z)) * (4. * s)


class _LutQuantize(torch.autograd.Function):
    """(q, idx int64) of a contiguous float32 / float64 device tensor; cfg = (mode, wrap, kind or None,
    lut, thresholds), s a device tensor [1] of x's dtype or None."""

    @staticmethod
    def forward(ctx, x, s, cfg):
        mode, wrap, kind, lut, thr = cfg
        if x.dtype == torch.float64:
            q, idx = _lut_forward_torch(x, lut, thr, mode, wrap)
            idx32 = idx
        else:
            q = torch.empty_like(x)
            idx32 = torch.empty(x.shape, dtype=torch.int32, device=x.device)
            d = _lut_desc(x.numel(), mode, wrap, 0, lut, thr)
            with torch.cuda.device(x.device):
                _lib.check(_lib.lib().thz_lut_quantize_forward(ctypes.byref(d), _p(x), _p(q), _p(idx32),
                                                               _stream_handle()))
            idx = idx32.long()
        ctx.mark_non_differentiable(idx)
        ctx.cfg = cfg
        if kind not in (None, _lib.LUTQ_GRAD_IDENTITY):
            ctx.save_for_backward(x, idx32, s)
        return q, idx

    @staticmethod
    def backward(ctx, g, _gidx):
        mode, wrap, kind, lut, thr = ctx.cfg
        if kind is None:
            return None, None, None
        if kind == _lib.LUTQ_GRAD_IDENTITY:  # Components/quantization.py:70-71 hands grad_output through
            return g, None, None
        x, idx32, s = ctx.saved_tensors
        g = g.to(x.dtype).contiguous()
        if x.dtype == torch.float64:
            return g * _lut_slope_torch(x, idx32, lut, kind, s), None, None
        out = torch.empty_like(x)
        d = _lut_desc(x.numel(), mode, wrap, kind, lut, ())
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().thz_lut_quantize_backward(ctypes.byref(d), _p(x), _p(idx32), _p(g), _p(s), _p(out),
                                                            _stream_handle()))
        return out, None, None


def _heightmap_input(x, who):
    if not torch.is_tensor(x):
        raise TypeError(f"{who}: the input must be a tensor")
    _require_device(x, who)
    if x.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{who}: kernels compute in float32 (float64 runs the torch op sequence); got {x.dtype}")
    return x.contiguous()


def lut_quantize(x, lut, *, mode="bucketize", wrap=False, midvals=None, surrogate="identity", s=1.0):
    """Snap ``x`` to the levels ``lut``: returns ``(q, idx)``, q = lut[idx] in x's shape and dtype, idx int64
    (not differentiable).

    ``mode="bucketize"``: nearest_neighbor_search / nearest_idx (utils/Helper_Functions.py:375-398):
    idx = torch.bucketize(x, midvals, right=True); ``midvals`` defaults to the float32 midpoints of
    neighbouring levels (lut_mid, :371-372) in x's precision and must ascend.  ``wrap=True`` then takes idx modulo
    len(midvals), the reference's own last step, which sends every x at or above the top threshold to
    level 0.  ``mode="argmin"``: the notebooks' ``quantization(input, lut)``: the first minimum of |x - lut|.
    Levels and thresholds are compared in float32 exactly as given: q and idx equal torch's bit for bit.

    ``surrogate``: the gradient handed to x -- "identity" (NearestNeighborSearch, Components/
    quantization.py:59-71), "poly" (:73-96), "sigmoid" (:98-122), or None for no gradient (the
    notebooks' post-hoc snap).  ``s`` is the steepness: a Python number, or a device tensor the
    backward kernel reads when it runs (a captured graph sees each replay's value).  Where the
    surrogates look up the "other end" lut[idx + sign(x - q)], index -1 reads the last level as in the
    reference, and an index one past the last level, where the reference raises, reads level 0.

    float32 tensors on the ROCm device run thz_lut_quantize_forward / _backward (one pass each);
    float64 device tensors run the reference's torch op sequence.  With ``lut`` and ``midvals`` given as
    lists or CPU tensors nothing syncs and the call is capturable in torch.cuda.graph.  A table given as
    a device tensor is read back to the host on every call (the levels travel by value in the kernel's
    descriptor): that waits for the stream, and inside a graph capture it raises RuntimeError."""
    who = "lut_quantize"
    if mode not in _LUT_MODES:
        raise ValueError(f"{who}: mode must be 'bucketize' or 'argmin', got {mode!r}")
    if surrogate is not None and surrogate not in _LUT_KINDS:
        raise ValueError(f"{who}: surrogate must be 'identity', 'poly', 'sigmoid' or None, got {surrogate!r}")
    x = _heightmap_input(x, who)
    lut = _table(lut, who, x.dtype)
    if not 1 <= len(lut) <= _lib.THZ_MAX_LUT:
        raise ValueError(f"{who}: {len(lut)} levels; the kernels take 1 .. {_lib.THZ_MAX_LUT}")
    thr = ()
    if mode == "bucketize":
        thr = _lut_mid(lut, x.dtype) if midvals is None else _table(midvals, who, x.dtype)
        lo, hi = (1, len(lut)) if wrap else (0, len(lut) - 1)
        if not lo <= len(thr) <= hi:
            raise ValueError(f"{who}: {len(thr)} thresholds for {len(lut)} levels (wrap={bool(wrap)}: {lo} .. {hi})")
    kind = None if surrogate is None else _LUT_KINDS[surrogate]
    s_dev = None
    if kind in (_lib.LUTQ_GRAD_POLY, _lib.LUTQ_GRAD_SIGMOID):
        if torch.is_tensor(s) and s.is_cuda:
            s_dev = s.detach().to(x.dtype).reshape(1)
        else:
            s_dev = torch.full((1,), float(s), dtype=x.dtype, device=x.device)
    cfg = (_LUT_MODES[mode], bool(wrap), kind, lut, thr)
    if kind is None:
        with torch.no_grad():
            return _LutQuantize.apply(x.detach(), None, cfg)
    return _LutQuantize.apply(x, s_dev, cfg)


def _center_difference_torch(x):
    """utils/Helper_Functions.py:56-70 on [N, H, W]."""
    dx, dy = torch.zeros_like(x), torch.zeros_like(x)
    _, H, W = x.shape
    dx[:, :, 1:-1] = W / 4 * (-x[:, :, 0:-2] + 2 * x[:, :, 1:-1] - x[:, :, 2:])
    dy[:, 1:-1, :] = H / 4 * (-x[:, 0:-2, :] + 2 * x[:, 1:-1, :] - x[:, 2:, :])
    return dx, dy


def _tv_backward(x, gdx, gdy, grad_loss, shape):
    N, H, W = shape
    grad = torch.empty(shape, dtype=torch.float32, device=(x if x is not None else gdx).device)
    with torch.cuda.device(grad.device):
        _lib.check(_lib.lib().thz_tv_backward(_p(x), _p(gdx), _p(gdy), _p(grad_loss), N, H, W, _p(grad),
                                              _stream_handle()))
    return grad


class _CenterDifference(torch.autograd.Function):
    """dx, dy of a contiguous float32 [N, H, W]."""

    @staticmethod
    def forward(ctx, x):
        N, H, W = x.shape
        dx, dy = torch.empty_like(x), torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().thz_tv_forward(_p(x), N, H, W, _p(dx), _p(dy), None, None, 0, _stream_handle()))
        ctx.shape = (N, H, W)
        return dx, dy

    @staticmethod
    def backward(ctx, gdx, gdy):
        return _tv_backward(None, gdx.float().contiguous(), gdy.float().contiguous(), None, ctx.shape)


class _TotalVariation(torch.autograd.Function):
    """mean |dx| + mean |dy| of a contiguous float32 [N, H, W], a 0-d tensor."""

    @staticmethod
    def forward(ctx, x):
        N, H, W = x.shape
        tv = torch.empty((), dtype=torch.float32, device=x.device)
        nbytes = ctypes.c_size_t(0)
        _lib.check(_lib.lib().thz_tv_workspace_size(N, H, W, ctypes.byref(nbytes)))
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().thz_tv_forward(_p(x), N, H, W, None, None, _p(tv), _p(ws), ws.numel(),
                                                 _stream_handle()))
        ctx.save_for_backward(x)
        return tv

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        return _tv_backward(x, None, None, g.float().reshape(1), tuple(x.shape))


def _planes(x, who):
    if x.dim() < 2:
        raise ValueError(f"{who}: the input needs the two spatial dimensions last; got shape {tuple(x.shape)}")
    if x.numel() == 0:
        raise ValueError(f"{who}: empty input {tuple(x.shape)}")
    return x.reshape(-1, x.shape[-2], x.shape[-1])


def center_difference(x):
    """center_difference (utils/Helper_Functions.py:56-70): ``(dx, dy)`` in x's shape,
    dx = W / 4 (-x[j-1] + 2 x[j] - x[j+1]) on the interior columns and 0 on the border, dy alike with H / 4
    on the interior rows (the last two dimensions are the spatial ones).  float32 on the ROCm device: one
    pass that reads x once and writes both maps (thz_tv_forward); the backward gathers the adjoint
    stencil of the two cotangents (thz_tv_backward).  float64 runs the torch op sequence."""
    x = _heightmap_input(x, "center_difference")
    p = _planes(x, "center_difference")
    dx, dy = _center_difference_torch(p) if x.dtype == torch.float64 else _CenterDifference.apply(p)
    return dx.reshape(x.shape), dy.reshape(x.shape)


def total_variation(x):
    """total_variation (utils/Helper_Functions.py:40-54): mean |dx| + mean |dy| of center_difference over
    every element, borders included, as a 0-d tensor; a 6-D [B, T, P, C, H, W] input is taken as
    [B T P, C, H, W] as the reference does.  float32 on the ROCm device: one pass that reads x once and
    forms the two sums as fp64 partials per workgroup added in a fixed order (thz_tv_forward; the same
    input gives the same bits); the backward recomputes sign(dx), sign(dy) from x and gathers their
    adjoint stencil, sign(0) = 0 (thz_tv_backward).  No host sync; float64 runs the torch op sequence."""
    x = _heightmap_input(x, "total_variation")
    p = _planes(x, "total_variation")
    if x.dtype == torch.float64:
        dx, dy = _center_difference_torch(p)
        return dx.abs().mean() + dy.abs().mean()
    return _TotalVariation.apply(p)


# -------------------------------------------------------------------------------------------------
# Measurement kernels (thz_metrics.hip) behind utils/metrics.py
# -------------------------------------------------------------------------------------------------
RegionStats = collections.namedtuple("RegionStats", "power moment1 moment2 peak argmax count")
LineWidths = collections.namedtuple("LineWidths", "peak argmax left right width")

_METRICS_DTYPES = {torch.complex64: _lib.METRICS_C64, torch.complex128: _lib.METRICS_C128,
                   torch.float32: _lib.METRICS_F32, torch.float64: _lib.METRICS_F64}
_REGION_KINDS = {"circ": _lib.REGION_CIRC, "rect": _lib.REGION_RECT}


def _region_table(regions, kind, who, device):
    """``(K, host table, device table)``: a ctypes array of thz_region for a list / CPU tensor (checked
    here), or a [K, 5] float32 device tensor in thz_region's layout for a device tensor (built by device
    copies and fills: no host read, so its values are not checked)."""
    on_device = torch.is_tensor(regions) and regions.is_cuda
    if on_device:
        if regions.device != device:
            raise ValueError(f"{who}: regions on {regions.device}, the input on {device}")
        if regions.is_complex() or regions.dtype == torch.bool:
            raise TypeError(f"{who}: regions must be real numbers; got {regions.dtype}")
        rows = regions.detach()
    else:
        rows = torch.as_tensor(regions, dtype=torch.float64) if not torch.is_tensor(regions) else regions.detach().double()
    if rows.numel() == 0:
        rows = rows.reshape(0, 3)
    if rows.dim() != 2 or rows.shape[1] not in (3, 4):
        raise ValueError(f"{who}: regions must be [K, 3] (cr, cc, a) or [K, 4] (cr, cc, a, b) in pixels; "
                         f"got shape {tuple(rows.shape)}")
    K, cols = int(rows.shape[0]), int(rows.shape[1])
    if K > _lib.THZ_MAX_REGIONS:
        raise ValueError(f"{who}: {K} regions; the kernel takes 0 .. {_lib.THZ_MAX_REGIONS} per call")
    kinds = [kind] * K if isinstance(kind, str) else list(kind)
    if len(kinds) != K or any(k not in _REGION_KINDS for k in kinds):
        raise ValueError(f"{who}: kind must be 'circ' or 'rect', or one of them per region ({K}); got {kind!r}")
    if cols == 3 and "rect" in kinds:
        raise ValueError(f"{who}: a rectangle needs [K, 4] regions (cr, cc, a, b)")
    codes = [_REGION_KINDS[k] for k in kinds]
    if on_device:
        tab = torch.zeros((K, 5), dtype=torch.float32, device=device)
        if K:
            tab[:, 1:1 + cols] = rows.to(torch.float32)
            as_int = tab.view(torch.int32)
            for k, code in enumerate(codes):
                if code:
                    as_int[k, 0] = code
        return K, None, tab
    vals = rows.tolist()
    for k, r in enumerate(vals):
        if not all(math.isfinite(v) for v in r) or any(v < 0 for v in r[2:]):
            raise ValueError(f"{who}: region {k} = {r}: centre and sizes must be finite, sizes >= 0")
    host = (_lib.Region * max(1, K))(*[_lib.Region(kind=c, cr=r[0], cc=r[1], a=r[2], b=r[3] if cols == 4 else 0.0)
                                       for c, r in zip(codes, vals)])
    return K, host, None


def _region_desc(x, K, host, dev):
    N, H, W = x.shape
    table = dev.data_ptr() if dev is not None else (ctypes.addressof(host) if K else 0)
    return _lib.RegionStatsDesc(N=N, H=H, W=W, dtype=_METRICS_DTYPES[x.dtype], K=K, regions=table,
                                regions_on_device=int(dev is not None))


class _RegionStats(torch.autograd.Function):
    """The statistics of a contiguous [N, H, W] field or intensity; the five sums are differentiable."""

    @staticmethod
    def forward(ctx, x, table):
        K, host, dev = table
        d = _region_desc(x, K, host, dev)
        out = torch.empty((x.shape[0], K + 1, 8), dtype=torch.float64, device=x.device)
        nbytes = ctypes.c_size_t(0)
        _lib.check(_lib.lib().thz_region_stats_workspace_size(ctypes.byref(d), ctypes.byref(nbytes)))
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().thz_region_stats_forward(ctypes.byref(d), _p(x), _p(out), _p(ws), ws.numel(),
                                                           _stream_handle()))
        ctx.save_for_backward(x)
        ctx.table = table
        stats = (out[..., 0].contiguous(), out[..., 1:3].contiguous(), out[..., 3:5].contiguous(),
                 out[..., 5].contiguous(), out[..., 6].to(torch.int64), out[..., 7].to(torch.int64))
        ctx.mark_non_differentiable(*stats[3:])
        return stats

    @staticmethod
    def backward(ctx, g_power, g_m1, g_m2, *_):
        x, = ctx.saved_tensors
        K, host, dev = ctx.table
        G = torch.stack((g_power, g_m1[..., 0], g_m1[..., 1], g_m2[..., 0], g_m2[..., 1]), dim=-1).double().contiguous()
        grad = torch.empty_like(x)
        d = _region_desc(x, K, host, dev)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().thz_region_stats_backward(ctypes.byref(d), _p(x), _p(G), _p(grad), _stream_handle()))
        return grad, None


def region_stats(x, regions, kind="circ"):
    """Power, moments and peak of every region of every plane in one pass (thz_region_stats_forward).

    ``x``: a complex64 / complex128 field (I = |x|^2, formed in float64) or a float32 / float64 intensity on
    the ROCm device, the two spatial dimensions last.  ``regions``: [K, 3] rows (cr, cc, a) or [K, 4] rows
    (cr, cc, a, b), 0 <= K <= 16, in pixel units (row, column), as a list, a CPU tensor or a device tensor;
    ``kind``: "circ" ((i - cr)^2 + (j - cc)^2 <= a^2) or "rect" (|i - cr| <= a and |j - cc| <= b), or a list
    with one of them per region.  The values are taken as float32 and the tests made in float64.  A list or
    CPU tensor is checked here and travels by value in the launch; a device tensor is read by the kernel (no
    host read, so it is not checked).  Region index K of the result is the whole plane.

    Returns ``RegionStats`` of float64 tensors shaped ``x.shape[:-2] + (K + 1,)``: ``power`` = sum I,
    ``moment1`` [..., 2] = (sum I i, sum I j), ``moment2`` [..., 2] = (sum I i^2, sum I j^2), ``peak`` = max I,
    ``argmax`` (int64, the lowest flat index i W + j that attains the peak; -1 and peak 0 for a region with
    no pixel in the plane) and ``count`` (int64, pixels inside).  power, moment1 and moment2 are differentiable
    in x through one backward pass (thz_region_stats_backward); peak, argmax and count are not.  Sums are
    float64 in a fixed order: the same input gives the same bits.  No host sync; capturable in
    torch.cuda.graph."""
    who = "region_stats"
    if not torch.is_tensor(x):
        raise TypeError(f"{who}: the input must be a tensor")
    _require_device(x, who)
    if x.dtype not in _METRICS_DTYPES:
        raise TypeError(f"{who}: complex64 / complex128 fields or float32 / float64 intensities; got {x.dtype}")
    p = _planes(x.resolve_conj().contiguous(), who)
    table = _region_table(regions, kind, who, x.device)
    stats = _RegionStats.apply(p, table)
    lead = tuple(x.shape[:-2])
    return RegionStats(*[t.reshape(lead + tuple(t.shape[1:])) for t in stats])


def line_widths(x, level=0.5):
    """Peak and width at ``level`` x peak of every line along the last dimension (thz_line_widths).

    ``x``: float32 / float64 on the ROCm device.  Returns ``LineWidths`` shaped ``x.shape[:-1]``: ``peak``,
    ``argmax`` (int64, the lowest index of the peak), ``left``, ``right`` and ``width`` = right - left
    (float64, in samples): the crossings of t = level x peak nearest to the peak on either side, linearly
    interpolated in float64 between the last sample below t and its neighbour towards the peak.  A side
    that never falls below t before the edge gives NaN there and for the width.  Not differentiable; no host
    sync; capturable in torch.cuda.graph."""
    who = "line_widths"
    if not torch.is_tensor(x):
        raise TypeError(f"{who}: the input must be a tensor")
    _require_device(x, who)
    if x.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{who}: float32 / float64 lines; got {x.dtype}")
    if x.dim() < 1 or x.numel() == 0:
        raise ValueError(f"{who}: empty input {tuple(x.shape)}")
    level = float(level)
    if not 0.0 < level < 1.0:
        raise ValueError(f"{who}: level must lie in (0, 1); got {level}")
    v = x.detach().contiguous()
    W = v.shape[-1]
    out = torch.empty((v.numel() // W, 5), dtype=torch.float64, device=v.device)
    with torch.cuda.device(v.device):
        _lib.check(_lib.lib().thz_line_widths(_p(v), _METRICS_DTYPES[v.dtype], out.shape[0], W, level, _p(out),
                                              _stream_handle()))
    out = out.reshape(tuple(v.shape[:-1]) + (5,))
    return LineWidths(out[..., 0], out[..., 1].to(torch.int64), out[..., 2], out[..., 3], out[..., 4])


# -------------------------------------------------------------------------------------------------
# IFTA projections (thz_ifta.hip) behind ifta.py
# -------------------------------------------------------------------------------------------------
IFTA_STATS = ("S_all", "S_in", "S_TU", "S_TT", "s", "eff")  # the columns of ifta_target_stats


def _ifta_planes(U, who):
    """The field as contiguous [N, H, W] complex64 planes on the device."""
    if not torch.is_tensor(U):
        raise TypeError(f"{who}: the field must be a tensor")
    _require_device(U, who)
    if U.dtype == torch.complex128:
        raise TypeError(f"{who}: the IFTA kernels compute in complex64; got a complex128 field -- cast it to "
                        "complex64")
    if U.dtype != torch.complex64:
        raise TypeError(f"{who}: a complex64 field; got {U.dtype}")
    return _planes(U.resolve_conj().contiguous(), who)


def _ifta_target(T, mask, planes, who):
    """(T float32 contiguous, its plane count 1 or N, mask uint8 [H, W] or None) for [N, H, W] planes."""
    N, H, W = planes.shape
    if not torch.is_tensor(T) or T.is_complex() or T.device != planes.device:
        raise TypeError(f"{who}: the target amplitude must be a real tensor on {planes.device}")
    if T.dim() < 2 or tuple(T.shape[-2:]) != (H, W) or T.numel() not in (H * W, N * H * W):
        raise ValueError(f"{who}: target {tuple(T.shape)} for planes {(N, H, W)}: [H, W] or one per plane")
    T = T.detach().to(torch.float32).contiguous()
    if mask is not None:
        if not torch.is_tensor(mask) or mask.device != planes.device or mask.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"{who}: the window mask must be a bool / uint8 tensor on {planes.device}")
        if tuple(mask.shape) != (H, W):
            raise ValueError(f"{who}: window mask {tuple(mask.shape)} for planes of {(H, W)}")
        mask = mask.contiguous()
        mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    return T, (1 if T.numel() == H * W else N), mask


def ifta_target_stats(U, T, mask=None, out=None):
    """The sums one IFTA iteration needs of the planes ``U`` against the target amplitude ``T``, in one pass
    (thz_ifta_target_stats).

    ``U``: complex64 [..., H, W] on the ROCm device (N planes).  ``T``: real, [H, W] for every plane or one per
    plane, non-negative.  ``mask``: bool / uint8 [H, W], the signal window; None: every pixel.  Returns float64
    [N, 6] = (S_all = sum |U|^2, S_in = sum_M |U|^2, S_TU = sum_M T |U|, S_TT = sum_M T^2, s = S_TU / S_TT,
    eff = S_in / S_all), quotients 0 where the denominator is 0; ``s`` is the least-squares scale of s T against
    |U| on the window.  ``out``: a contiguous float64 [N, 6] device tensor (a row of a history array) to write
    instead.  Sums are float64 in a fixed order: the same input gives the same bits.  No autograd, no host sync;
    capturable in torch.cuda.graph."""
    who = "ifta_target_stats"
    p = _ifta_planes(U, who)
    T, tp, mask = _ifta_target(T, mask, p, who)
    N, H, W = p.shape
    if out is None:
        out = torch.empty((N, 6), dtype=torch.float64, device=p.device)
    elif (not torch.is_tensor(out) or out.dtype != torch.float64 or out.device != p.device or not out.is_contiguous()
          or tuple(out.shape) != (N, 6)):
        raise ValueError(f"{who}: out must be a contiguous float64 [{N}, 6] tensor on {p.device}")
    d = _lib.IftaDesc(N=N, H=H, W=W, target_planes=tp, alpha=1.0, beta=1.0)
    nbytes = ctypes.c_size_t(0)
    _lib.check(_lib.lib().thz_ifta_target_stats_workspace_size(ctypes.byref(d), ctypes.byref(nbytes)))
    ws = torch.empty(max(1, nbytes.value), dtype=torch.uint8, device=p.device)
    with torch.cuda.device(p.device):
        _lib.check(_lib.lib().thz_ifta_target_stats(ctypes.byref(d), _p(p), _p(T), _p(mask), _p(out), _p(ws),
                                                    ws.numel(), _stream_handle()))
    return out


def ifta_target_project(U, T, scale, mask=None, alpha=1.0, beta=1.0, out=None):
    """Impose the target amplitude on the planes ``U`` (thz_ifta_target_project): inside the window
    a' = max(0, alpha s T + (1 - alpha) |U|) with U's phase (a' itself where U = 0), outside it beta U.

    ``U``, ``T``, ``mask`` as ``ifta_target_stats``.  ``scale``: float64 device tensor, one value per plane
    (column ``s`` of the stats, or a joint scale), read by the kernel.  ``alpha`` in (0, 2]: 1 is
    Gerchberg-Saxton, above 1 the over-compensated form; ``beta`` in [0, 1]: 1 leaves the amplitude outside the
    window free, 0 suppresses it.  ``out``: a contiguous complex64 tensor of U's shape; ``out=U`` projects in
    place.  Returns the projected planes in U's shape.  No autograd, no host sync; capturable."""
    who = "ifta_target_project"
    alpha, beta = float(alpha), float(beta)
    if not 0.0 < alpha <= 2.0:
        raise ValueError(f"{who}: alpha must lie in (0, 2]; got {alpha}")
    if not 0.0 <= beta <= 1.0:
        raise ValueError(f"{who}: beta must lie in [0, 1]; got {beta}")
    if out is not None and out is U and not U.is_contiguous():
        raise ValueError(f"{who}: in place needs a contiguous field")
    p = _ifta_planes(U, who)
    T, tp, mask = _ifta_target(T, mask, p, who)
    N, H, W = p.shape
    if (not torch.is_tensor(scale) or scale.dtype != torch.float64 or scale.device != p.device
            or scale.numel() != N):
        raise ValueError(f"{who}: scale must be a float64 tensor of {N} values on {p.device}")
    scale = scale.detach().reshape(-1).contiguous()
    if out is None:
        out = torch.empty_like(p)
    elif (not torch.is_tensor(out) or out.dtype != torch.complex64 or out.device != p.device
          or not out.is_contiguous() or out.numel() != p.numel()):
        raise ValueError(f"{who}: out must be a contiguous complex64 tensor of {tuple(U.shape)} on {p.device}")
    d = _lib.IftaDesc(N=N, H=H, W=W, target_planes=tp, alpha=alpha, beta=beta)
    with torch.cuda.device(p.device):
        _lib.check(_lib.lib().thz_ifta_target_project(ctypes.byref(d), _p(p), _p(T), _p(mask), _p(scale), _p(out),
                                                      _stream_handle()))
    return out.reshape(U.shape)


def _ifta_doe_desc(N, H, W, doe_shape, wavelength, eps, lut, incident_planes, who="ifta_doe_project"):
    hs, ws = int(doe_shape[0]), int(doe_shape[1])
    if hs < 1 or ws < 1 or H % hs or W % ws:
        raise ValueError(f"{who}: a {H} x {W} field over {hs} x {ws} cells: every cell must be a whole number of "
                         "field pixels")
    if not 1 <= len(lut) <= _lib.THZ_MAX_LUT:
        raise ValueError(f"{who}: {len(lut)} levels; the kernels take 1 .. {_lib.THZ_MAX_LUT}")
    d = _lib.IftaDoeDesc(N=N, H=H, W=W, hs=hs, ws=ws, incident_planes=incident_planes, wavelength=float(wavelength),
                         epsilon=float(eps), L=len(lut))
    for i, v in enumerate(lut):
        d.lut[i] = v
    return d


def ifta_doe_project(U, doe_shape, wavelength, eps, lut, q=1.0, incident=None):
    """Turn the back-propagated field ``U`` into a height map on the level table (thz_ifta_doe_project).

    ``U``: complex64 [..., H, W] (N fields); ``doe_shape`` = (hs, ws) cells, each a whole number r_h x r_w of
    field pixels.  ``incident``: the field A that lit the DOE, complex64 [H, W] or one per field; None: 1.  Per
    cell g = sum U conj(A) (float64, row-major), h_c = (-arg g / kappa - base plane) mod h_max with kappa =
    2 pi / wavelength (sqrt(eps) - 1) and h_max = 2 pi / kappa, then the nearest level of ``lut`` (ascending in
    [0, h_max)) on the circle, the lowest index on a tie; the cell takes it when its cyclic distance is at most
    ``q`` times half the gap to the neighbouring level on its side, and keeps h_c otherwise.  ``q`` in [0, 1]: a
    Python number, or a float32 device tensor [1] the kernel reads when it runs (a captured graph sees each
    replay's value); 0 leaves the map continuous, 1 snaps every cell.  ``lut``: a list or CPU tensor; a device
    tensor is read back on every call and refused during a graph capture, as ``lut_quantize`` does.  The loss
    tangent takes no part.

    Returns ``(h, idx)``: float32 and int32 [..., hs, ws]; idx is the level, -1 where the cell kept h_c.  No
    autograd, no host sync with a host table; capturable."""
    who = "ifta_doe_project"
    p = _ifta_planes(U, who)
    N, H, W = p.shape
    lut = _table(lut, who, torch.float32)
    planes = 0
    if incident is not None:
        if not torch.is_tensor(incident) or incident.device != p.device:
            raise TypeError(f"{who}: the incident field must be a tensor on {p.device}")
        if incident.dtype != torch.complex64:
            raise TypeError(f"{who}: the IFTA kernels compute in complex64; got an incident field of {incident.dtype}")
        if incident.dim() < 2 or tuple(incident.shape[-2:]) != (H, W) or incident.numel() not in (H * W, N * H * W):
            raise ValueError(f"{who}: incident field {tuple(incident.shape)} for {(N, H, W)}: [H, W] or one per field")
        incident = incident.detach().resolve_conj().contiguous()
        planes = 1 if incident.numel() == H * W else N
    d = _ifta_doe_desc(N, H, W, doe_shape, wavelength, eps, lut, planes, who)
    if torch.is_tensor(q):
        if not q.is_cuda or q.dtype != torch.float32 or q.numel() != 1 or q.device != p.device:
            raise ValueError(f"{who}: q as a tensor must be one float32 value on {p.device}")
        q_dev = q.detach()
    else:
        if not 0.0 <= float(q) <= 1.0:
            raise ValueError(f"{who}: q must lie in [0, 1]; got {q}")
        q_dev = torch.full((1,), float(q), dtype=torch.float32, device=p.device)
    lead = tuple(U.shape[:-2])
    h = torch.empty(lead + (d.hs, d.ws), dtype=torch.float32, device=p.device)
    idx = torch.empty(lead + (d.hs, d.ws), dtype=torch.int32, device=p.device)
    with torch.cuda.device(p.device):
        _lib.check(_lib.lib().thz_ifta_doe_project(ctypes.byref(d), _p(p), _p(incident), _p(q_dev), _p(h), _p(idx),
                                                   _stream_handle()))
    return h, idx


# ---------------------------------------------------------------------------------------------
# Thick-element DOE: split-step propagation through the relief (thz_thick.hip)
# ---------------------------------------------------------------------------------------------
THICK_CONVENTIONS = {"reference": -1.0, "physical": 1.0}
_THICK_MAX_SLICES = 256
_THICK_BASE_PLANE = float(np.float32(2e-3))  # DOE_BASE_PLANE (csrc/thz_dev.hpp), BASE_PLANE_THICKNESS of the layers


def thick_doe_native(H, W, pad_h, pad_w, slices):
    """True where thz_thick_forward serves the geometry: padded sides that are powers of two from 64 to
    8192 (they may differ) and at most 256 slices."""
    def pow2(n):
        return 64 <= n <= 8192 and n & (n - 1) == 0
    return pow2(H + 2 * pad_h) and pow2(W + 2 * pad_w) and slices <= _THICK_MAX_SLICES


def _thick_desc(field, height, wavelengths, spacing, eps, tand, thickness, slices, pad_h, pad_w, bl, sign):
    B, C, H, W = field.shape
    wl = _lib.float_array(wavelengths)
    d = _lib.ThickDesc(B=B, C=C, H=H, W=W, pad_h=pad_h, pad_w=pad_w, bandlimit=bl, hs=height.shape[0],
                       ws=height.shape[1], slices=slices, thickness=thickness, dx=float(spacing[0]),
                       dy=float(spacing[1]), epsilon=float(eps), tand=float(tand), phase_sign=sign,
                       wavelengths=_fptr(wl))
    d._keep = wl
    return d


def _thick_fused(field, height, *args, stash=None):
    """thz_thick_forward, or thz_thick_forward_saved into ``stash`` [B, C, H, W] complex64."""
    d = _thick_desc(field, height, *args)
    out = torch.empty_like(field)
    L = _lib.lib()
    from .propagation import _launch
    if stash is None:
        _launch(L.thz_thick_workspace_size, L.thz_thick_forward, d, field.device, field, height, out)
    else:
        _launch(L.thz_thick_workspace_size, L.thz_thick_forward_saved, d, field.device, field, height, out, stash)
    return out


class _ThickFused(torch.autograd.Function):
    """thick_doe(grad="fused"): the fused forward (the saving one when the map requires grad) and
    thz_thick_backward, which forms no slab field and keeps one stash: V_s where slab s is the pixel's active one."""

    @staticmethod
    def forward(ctx, field, height, args):
        x, h = field.detach().resolve_conj().contiguous(), height.detach().contiguous()  # the kernels read memory
        need_h = ctx.needs_input_grad[1]
        stash = torch.empty_like(x) if need_h else None
        out = _thick_fused(x, h, *args, stash=stash)
        ctx.args, ctx.shape = args, tuple(x.shape)
        ctx.save_for_backward(h, stash)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        h, stash = ctx.saved_tensors
        need_x, need_h = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_x or need_h):
            return None, None, None
        g = grad_out.resolve_conj().contiguous()
        if g.dtype != torch.complex64:
            raise TypeError(f"thick_doe backward: grad_out must be complex64; got {g.dtype}")
        d = _thick_desc(g, h, *ctx.args)
        gx = torch.empty_like(g) if need_x else None
        gh = torch.empty_like(h) if need_h else None
        L = _lib.lib()
        from .propagation import _launch
        _launch(L.thz_thick_backward_workspace_size, L.thz_thick_backward, d, g.device, g, h, stash, gx, gh)
        return gx, gh, None


def _thick_compose(field, height, wavelengths, spacing, eps, tand, thickness, slices, pad_h, pad_w, bl, sign):
    from . import doe, propagation
    dz = float(np.float32(thickness)) / slices  # the library's dz: the fp32 thickness over S, in double
    u = field
    for s in range(slices):
        d = (height - s * dz).clamp(0.0, dz)
        if s > 0:
            d = d - _THICK_BASE_PLANE  # the modulate kernel adds the base plate to its argument
        # sign = +1: U conj(t) = conj(conj(U) t); the kernels read memory, so the conjugates are formed
        u = doe.modulate(u.conj().resolve_conj() if sign > 0 else u, d, wavelengths, eps, tand)[0]
        u = propagation.asm_propagate(u.conj().resolve_conj() if sign > 0 else u, wavelengths, spacing, [dz], pad_h,
                                      pad_w, True, bl)[0]
    return u


def thick_doe(field, height, wavelengths, spacing, eps, tand, thickness, slices, padding_scale=1, bandlimit="exact",
              convention="reference", method="auto", grad=None):
    """The field behind a DOE of finite thickness: split-step (multi-slice) propagation through the relief.

    ``field`` complex64 [B, C, H, W]; ``height`` float32 [hs, ws], nearest-upsampled to [H, W]; ``thickness`` T
    > 0 and ``slices`` S >= 1.  With dz = T / S and d_s = clamp(h - s dz, 0, dz) (d_0 also carries the base
    plate), slab s multiplies by t_s = exp(-k/2 d_s tand sqrt(eps)) exp(sigma i k d_s (sqrt(eps) - 1)) and
    ASM_prop(z_distance=dz, padding_scale, bandlimit) carries the field to the next slab, cropped every step.
    The result is the field in the plane T above the base plate; heights above T count as T, below 0 as 0.

    ``convention``: "reference" (sigma = -1, DOELayer.modulate's sign: S = 1 is modulate then ASM over T) or
    "physical" (sigma = +1, consistent with the ASM's exp(+i z k_z)).  ``bandlimit``: "exact", "approx" or None.
    ``method``: "fused" -- the thz_thick.hip kernels, two launches per slab, capturable, forward only unless
    ``grad`` says otherwise; padded sides must be powers of two from 64 to 8192 and S <= 256.  "compose" -- the same model as a loop over doe.modulate
    and the ASM kernels, differentiable in the field and the map.  "auto": fused where it serves the geometry and
    nothing requires grad, else compose.

    ``grad``: None -- as above.  "fused" -- the gradient of the fused path is the native backward
    (thz_thick_backward): "fused" and, on a geometry the kernels serve, "auto" then stay on the fused kernels when
    something requires grad; the forward keeps one field-sized stash instead of every slab's field.  "auto" on
    another geometry falls back to compose, method="fused" there raises the library's unsupported error, and
    method="compose" with grad="fused" is a ValueError.  The derivative in a height is taken inside the slab the
    height ends in; a height exactly on a slab face, on 0 or on T, below 0 or above T has gradient 0."""
    who = "thick_doe"
    if grad not in (None, "fused"):
        raise ValueError(f"{who}: grad must be None or 'fused'; got {grad!r}")
    if grad == "fused" and method == "compose":
        raise ValueError(f"{who}: grad='fused' is the backward of the fused kernels; method='compose' has autograd's")
    _require_device(field, who)
    if field.dtype != torch.complex64:
        raise TypeError(f"{who}: the DOE kernels compute in complex64; got {field.dtype}")
    if field.dim() != 4 or height.dim() != 2:
        raise ValueError(f"{who}: field [B, C, H, W] and height [hs, ws]; got {tuple(field.shape)}, {tuple(height.shape)}")
    if convention not in THICK_CONVENTIONS:
        raise ValueError(f"{who}: convention must be 'reference' or 'physical'; got {convention!r}")
    if method not in ("auto", "fused", "compose"):
        raise ValueError(f"{who}: method must be 'auto', 'fused' or 'compose'; got {method!r}")
    slices = int(slices)
    thickness = float(np.float32(thickness))
    if slices < 1 or not thickness > 0.0:
        raise ValueError(f"{who}: thickness > 0 and slices >= 1; got {thickness}, {slices}")
    from . import propagation
    B, C, H, W = field.shape
    wavelengths = [float(w) for w in wavelengths]
    if len(wavelengths) != C:
        raise ValueError(f"{who}: {len(wavelengths)} wavelengths for {C} channels")
    spacing = (float(spacing[0]), float(spacing[1])) if np.ndim(spacing) else (float(spacing), float(spacing))
    ps = padding_scale if np.ndim(padding_scale) else (padding_scale, padding_scale)
    pad_h, pad_w = propagation.asm_padding(H, W, ps)
    bl = propagation._bandlimit(bandlimit)
    sign = THICK_CONVENTIONS[convention]
    diff = torch.is_grad_enabled() and (field.requires_grad or height.requires_grad)
    native = thick_doe_native(H, W, pad_h, pad_w, slices)
    if method == "auto":
        method = "fused" if native and (not diff or grad == "fused") else "compose"
    height = height.to(device=field.device, dtype=torch.float32)
    args = (wavelengths, spacing, float(eps), float(tand), thickness, slices, pad_h, pad_w, bl, sign)
    if method == "compose":
        return _thick_compose(field, height, *args)
    if diff and grad == "fused":
        return _ThickFused.apply(field, height, args)
    if diff:
        raise RuntimeError(f"{who}: method='fused' is forward only unless grad='fused'; use that, or method='compose' "
                           "(or 'auto'), for gradients")
    return _thick_fused(field.detach().contiguous(), height.detach().contiguous(), *args)
