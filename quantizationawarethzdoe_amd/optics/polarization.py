"""Polarization analysis of a vectorial field (Addons/Polarization.py:45-92): Stokes vector and ellipse
parameters, one fused pass each (csrc/thz_optics.hip, the complex128 forms in csrc/thz_f64.hip).
"""
import torch

from .. import _lib
from .._call import _require_device, call

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
    call(entry, ex, ey, ex.numel(), *rest, device=ex.device)


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
