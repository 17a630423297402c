"""Detector noise models (Addons/Noise.py, utils/Noise.py, utils/Helper_Functions.py:258-366) on the fused
counter-based sampler (csrc/thz_noise.hip).
"""
import torch

from .. import _lib
from .._call import _require_device, call, workspace

NOISE_KINDS = {"gauss": _lib.NOISE_GAUSS, "uniform": _lib.NOISE_UNIFORM, "poisson": _lib.NOISE_POISSON,
               "poisson_gauss": _lib.NOISE_POISSON_GAUSS}


def _noise_kind(kind):
    try:
        return NOISE_KINDS[str(kind).lower()]
    except KeyError:
        raise ValueError(f"noise kind must be one of {sorted(NOISE_KINDS)}; got {kind!r}") from None


def noise_state(x, rng):
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
    call(_lib.lib().thz_noise_apply, d, x, out, x.numel(), device=x.device)


def _sum_workspace(x):
    return workspace(_lib.lib().thz_signal_scale_workspace_size, x.numel(), device=x.device)


def signal_scale(x, snr_linear):
    """sqrt(mean(|x|^2) / snr_linear) of a float32 / complex64 device tensor as a device scalar [1]
    (utils/Noise.py:28-32): summed in fp64 in a fixed order, rounded to fp32 once, no sync
    (thz_signal_scale)."""
    _require_device(x, "signal_scale")
    x = x.contiguous()
    scale = torch.empty(1, dtype=torch.float32, device=x.device)
    ws = _sum_workspace(x)
    call(_lib.lib().thz_signal_scale, x, x.numel(), int(x.is_complex()), float(snr_linear), scale, ws, ws.numel(),
         device=x.device)
    return scale


def noise_draws(what, rng, n, device=None):
    """The raw draws of elements 0 .. n-1 of rng = (state, stream) that the noise kernels use
    (thz_noise_draws): what = "normal" [n], "uniform" [n] or "complex_normal" [n] complex64."""
    state, stream = rng
    code = {"normal": _lib.DRAW_NORMAL, "uniform": _lib.DRAW_UNIFORM, "complex_normal": _lib.DRAW_COMPLEX_NORMAL}[what]
    _require_device(state, "noise_draws")
    out = torch.empty(2 * n if what == "complex_normal" else n, dtype=torch.float32, device=state.device)
    call(_lib.lib().thz_noise_draws, code, state, int(stream), int(n), out, device=state.device)
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
            call(_lib.lib().thz_snr_noise_backward, g, x, x.numel(), int(x.is_complex()), float(snr), scale[0], state,
                 stream, gx, ws, ws.numel(), device=x.device)
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
    state, stream = noise_state(x, rng)
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
    state, stream = noise_state(data, rng)
    return _Noise.apply(data, state, stream, (cfg[0], _lib.NOISE_IN_FIELD_INTENSITY) + cfg[1:])
