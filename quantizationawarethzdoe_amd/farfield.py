"""Far-field patterns and diffraction orders of a field, a module of this port alone like modes.py and points.py
(csrc/thz_farfield.hip).  Beam splitters, gratings, diffusers and hologram feeds are specified at infinity:
order efficiencies, a pattern cut in a phi-plane, a (u, v) map.  The far-field amplitude is a non-uniform DFT,

    A[b, c, m] = scale sum_ij U[b, c, i, j] exp(-2 pi i (s_c p_m x_j + s_c q_m y_i)),

whose kernel matrix separates per axis, so it is applied as complex products on the fp32 matrix cores with the table
tiles generated on the chip and never stored (the model and the numerical contract are stated in include/thzdoe.h).

Conventions, those of modes.py: ``spacing`` is a scalar or (dx, dy), ``center`` is (x0, y0) in metres from the plane's
centre pixel, x runs along the last dimension, pixel j of n sits at (j - (n - 1) / 2) pitch - x0.  ``space="cosine"``
takes direction cosines (u, v) = (sin theta cos phi, sin theta sin phi) and needs the wavelengths;
``space="frequency"`` takes spatial frequencies (fx, fy) in cycles per metre.  ``scale`` defaults to dx dy, the angular
spectrum.  ``obliquity=True`` (cosine space) multiplies by -i w / lambda_c, w = sqrt(max(0, 1 - u^2 - v^2)): the
Rayleigh-Sommerfeld far-field amplitude r E exp(-i k r).

Host directions (a list, numpy, a CPU tensor) are checked -- finite, u^2 + v^2 <= 1 in cosine space -- and uploaded, a
blocking copy; a float64 device tensor is taken as it is, unchecked, with no sync, so the call is capturable in
torch.cuda.graph once the channel factors of its wavelengths are on the device (first call).  A repeated call gives the
same bits, and B x C planes in one call the bits of the planes one at a time.
"""
import math

import torch

from . import _lib
from ._call import _require_device, call, workspace
from .modes import _pair, as_field

_FACTORS = {}  # (s_c ..., device index) -> double device [C]: uploaded once


def _factors(space, wavelengths, C, device, who):
    if space not in ("cosine", "frequency"):
        raise ValueError(f"{who}: space is 'cosine' or 'frequency'; got {space!r}")
    if space == "frequency":
        s = (1.0,) * C
    else:
        if wavelengths is None:
            raise ValueError(f"{who}: direction cosines need the wavelengths")
        wl = [float(x) for x in torch.as_tensor(wavelengths, dtype=torch.float64).reshape(-1).tolist()]
        if len(wl) != C:
            raise ValueError(f"{who}: {len(wl)} wavelengths for a field of {C} channels")
        if not all(x > 0 and math.isfinite(x) for x in wl):
            raise ValueError(f"{who}: wavelengths must be positive; got {wl}")
        s = tuple(1.0 / x for x in wl)
    key = (s, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _FACTORS:
        _FACTORS[key] = torch.tensor(s, dtype=torch.float64, device=device)
    return _FACTORS[key]


def _vector(v, cols, space, device, who, what):
    """a float64 device tensor [n] or [n, 2]: a device tensor as it is, host values checked and uploaded"""
    if torch.is_tensor(v) and v.is_cuda:
        if v.dtype != torch.float64:
            raise TypeError(f"{who}: device {what} are float64; got {v.dtype}")
        d = v.detach()
    else:
        d = torch.as_tensor(v).detach().to("cpu", torch.float64)
        if not bool(torch.isfinite(d).all()):
            raise ValueError(f"{who}: the {what} must be finite")
        if space == "cosine" and d.numel() and float((d * d).reshape(-1, cols).sum(-1).max()) > 1.0 + 1e-12:
            raise ValueError(f"{who}: direction cosines need u^2 + v^2 <= 1")
    if d.numel() == 0 or (cols == 2 and (d.dim() != 2 or d.shape[-1] != 2)) or (cols == 1 and d.dim() != 1):
        raise ValueError(f"{who}: {what} are {'[M, 2]' if cols == 2 else '[n]'}; got {tuple(d.shape)}")
    return d.to(device).contiguous()


def _field_args(field, spacing, wavelengths, who):
    if not torch.is_tensor(field) and hasattr(field, "data"):
        wavelengths = field.wavelengths_host if wavelengths is None else wavelengths
    return as_field(field, spacing, who) + (wavelengths,)


def _desc(shape, cfg, M=0, Mu=0, Mv=0):
    B, C, H, W = shape
    (dx, dy), (x0, y0), scale, obliquity = cfg
    return _lib.FarfieldDesc(B=B, C=C, H=H, W=W, M=M, Mu=Mu, Mv=Mv, obliquity=int(obliquity), dx=dx, dy=dy, x0=x0,
                             y0=y0, scale=scale)


def _cfg(spacing, center, scale, obliquity, space, who):
    if obliquity and space != "cosine":
        raise ValueError(f"{who}: the obliquity factor needs direction cosines (space='cosine')")
    dx, dy = spacing
    return (dx, dy), _pair(center, who, "center"), dx * dy if scale is None else float(scale), bool(obliquity)


class _ListForward(torch.autograd.Function):
    """A [B, C, M] of thz_farfield_list_forward; the sum is linear, so the backward is thz_farfield_list_adjoint."""

    @staticmethod
    def forward(ctx, field, dirs, s, cfg):
        ctx.saved, ctx.shape = (dirs, s, cfg), tuple(field.shape)
        d = _desc(field.shape, cfg, M=dirs.shape[0])
        out = torch.empty(*field.shape[:2], dirs.shape[0], dtype=torch.complex64, device=field.device)
        ws = workspace(_lib.lib().thz_farfield_workspace_size, d, 0, device=field.device)
        call(_lib.lib().thz_farfield_list_forward, d, field.contiguous(), dirs, s, out, ws, ws.numel(), device=field.device)
        return out

    @staticmethod
    def backward(ctx, g):
        return _ListAdjoint.apply(g.resolve_conj(), *ctx.saved, ctx.shape), None, None, None


class _ListAdjoint(torch.autograd.Function):
    """G [B, C, H, W] of thz_farfield_list_adjoint; its backward is thz_farfield_list_forward."""

    @staticmethod
    def forward(ctx, g, dirs, s, cfg, shape):
        ctx.saved = (dirs, s, cfg)
        out = torch.empty(shape, dtype=torch.complex64, device=g.device)
        call(_lib.lib().thz_farfield_list_adjoint, _desc(shape, cfg, M=dirs.shape[0]), g.contiguous(), dirs, s, out,
             device=g.device)
        return out

    @staticmethod
    def backward(ctx, g):
        return _ListForward.apply(g.resolve_conj(), *ctx.saved), None, None, None, None


def _grid(entry, x, shape, out_shape, u, v, s, cfg):
    d = _desc(shape, cfg, Mu=u.shape[0], Mv=v.shape[0])
    out = torch.empty(out_shape, dtype=torch.complex64, device=x.device)
    ws = workspace(_lib.lib().thz_farfield_workspace_size, d, 1, device=x.device)
    call(entry, d, x.contiguous(), u, v, s, out, ws, ws.numel(), device=x.device)
    return out


class _GridForward(torch.autograd.Function):
    """A [B, C, Mv, Mu] of thz_farfield_grid_forward; the backward is thz_farfield_grid_adjoint."""

    @staticmethod
    def forward(ctx, field, u, v, s, cfg):
        ctx.saved, ctx.shape = (u, v, s, cfg), tuple(field.shape)
        return _grid(_lib.lib().thz_farfield_grid_forward, field, field.shape,
                     (*field.shape[:2], v.shape[0], u.shape[0]), u, v, s, cfg)

    @staticmethod
    def backward(ctx, g):
        return _GridAdjoint.apply(g.resolve_conj(), *ctx.saved, ctx.shape), None, None, None, None


class _GridAdjoint(torch.autograd.Function):
    """G [B, C, H, W] of thz_farfield_grid_adjoint; its backward is thz_farfield_grid_forward."""

    @staticmethod
    def forward(ctx, g, u, v, s, cfg, shape):
        ctx.saved = (u, v, s, cfg)
        return _grid(_lib.lib().thz_farfield_grid_adjoint, g, shape, shape, u, v, s, cfg)

    @staticmethod
    def backward(ctx, g):
        return _GridForward.apply(g.resolve_conj(), *ctx.saved), None, None, None, None, None


def pattern(field, directions, spacing=None, wavelengths=None, center=(0.0, 0.0), space="cosine", obliquity=False,
            scale=None):
    """The far-field amplitude in arbitrary directions: ``field`` an ElectricField or complex64 [B, C, H, W] with
    ``spacing=`` (and ``wavelengths=`` in cosine space), ``directions`` [M, 2] -> complex64 [B, C, M]
    (thz_farfield_list_forward).  Gradients flow to the field (thz_farfield_list_adjoint), none to the directions.
    Conventions, checks and capture in the module's docstring."""
    who = "pattern"
    x, spacing, wavelengths = _field_args(field, spacing, wavelengths, who)
    cfg = _cfg(spacing, center, scale, obliquity, space, who)
    dirs = _vector(directions, 2, space, x.device, who, "directions")
    return _ListForward.apply(x.resolve_conj(), dirs, _factors(space, wavelengths, x.shape[1], x.device, who), cfg)


def pattern_grid(field, u, v, spacing=None, wavelengths=None, center=(0.0, 0.0), space="cosine", obliquity=False,
                 scale=None):
    """The far-field amplitude on the separable grid of directions (u[mu], v[mv]) -> complex64 [B, C, Mv, Mu]
    (thz_farfield_grid_forward: two chained passes, O(H W Mu + H Mu Mv) per plane).  A host grid is checked at its
    corners in cosine space; otherwise as ``pattern``.  Gradients flow to the field (thz_farfield_grid_adjoint)."""
    who = "pattern_grid"
    x, spacing, wavelengths = _field_args(field, spacing, wavelengths, who)
    cfg = _cfg(spacing, center, scale, obliquity, space, who)
    if space == "cosine" and not any(torch.is_tensor(a) and a.is_cuda for a in (u, v)):
        u, v = (torch.as_tensor(a).detach().to("cpu", torch.float64) for a in (u, v))
        if u.numel() and v.numel() and float(u.abs().max()) ** 2 + float(v.abs().max()) ** 2 > 1.0 + 1e-12:
            raise ValueError(f"{who}: direction cosines need u^2 + v^2 <= 1 over the whole grid")
    u, v = (_vector(a, 1, "frequency", x.device, who, what) for a, what in ((u, "u"), (v, "v")))
    return _GridForward.apply(x.resolve_conj(), u, v, _factors(space, wavelengths, x.shape[1], x.device, who), cfg)


def orders(field, period=None, mx=(-1, 0, 1), my=(0,), spacing=None, center=(0.0, 0.0)):
    """Diffraction efficiencies of a periodic field: float32 [B, C, len(my), len(mx)], |a|^2 of the order amplitudes
    a = 1 / (H W) sum U exp(-2 pi i (m x / Lx + n y / Ly)) at the orders m of ``mx`` and n of ``my``.  ``period`` is a
    scalar or (Lx, Ly) in metres; None takes the field's own extent (W dx, H dy).  The extent must be an integer number
    of periods (to 1e-9 relative), or the orders are not orthogonal and a ValueError is raised.  Summed over all H W
    orders of the extent the efficiencies give mean |U|^2.  Uses the grid kernels; gradients flow to the field."""
    who = "orders"
    x, (dx, dy) = as_field(field, spacing, who)
    H, W = x.shape[-2:]
    Lx, Ly = (W * dx, H * dy) if period is None else _pair(period, who, "period")
    for extent, L in ((W * dx, Lx), (H * dy, Ly)):
        if not (L > 0 and abs(extent / L - round(extent / L)) <= 1e-9 * (extent / L) and round(extent / L) >= 1):
            raise ValueError(f"{who}: the extent {extent} m is not an integer number of periods of {L} m")
    fx = torch.tensor([int(m) / Lx for m in mx], dtype=torch.float64)
    fy = torch.tensor([int(n) / Ly for n in my], dtype=torch.float64)
    a = pattern_grid(x, fx, fy, (dx, dy), None, center, "frequency", False, 1.0 / (H * W))
    return a.real.square() + a.imag.square()


def plane_waves(amplitudes, directions, shape, spacing, wavelengths=None, center=(0.0, 0.0), space="cosine"):
    """A sum of plane waves: ``amplitudes`` complex64 [B, C, M] in ``directions`` [M, 2] -> complex64 [B, C, H, W] with
    ``shape`` = (H, W), U[i, j] = sum_m a[m] exp(+2 pi i (s_c p_m x_j + s_c q_m y_i)): the list adjoint used as a
    synthesis, at scale 1 (thz_farfield_list_adjoint).  Gradients flow to the amplitudes."""
    who = "plane_waves"
    if not torch.is_tensor(amplitudes):
        raise TypeError(f"{who}: amplitudes must be a tensor")
    _require_device(amplitudes, who)
    if amplitudes.dtype == torch.complex128:
        raise TypeError(f"{who}: the kernels compute in complex64; got complex128 amplitudes -- cast them, an fp64 "
                        "variant does not exist")
    if amplitudes.dtype != torch.complex64 or amplitudes.dim() != 3:
        raise TypeError(f"{who}: amplitudes are complex64 [B, C, M]; got {amplitudes.dtype} {tuple(amplitudes.shape)}")
    B, C, M = amplitudes.shape
    H, W = int(shape[-2]), int(shape[-1])
    dirs = _vector(directions, 2, space, amplitudes.device, who, "directions")
    if dirs.shape[0] != M:
        raise ValueError(f"{who}: {M} amplitudes for {dirs.shape[0]} directions")
    cfg = _cfg(_pair(spacing, who, "spacing"), center, 1.0, False, space, who)
    s = _factors(space, wavelengths, C, amplitudes.device, who)
    return _ListAdjoint.apply(amplitudes.resolve_conj(), dirs, s, cfg, (B, C, H, W))


def axis_table(n_pix, pitch, centre, p, wavelengths=None, space="cosine", device="cuda"):
    """complex64 [C, M, n_pix]: one axis' table exp(-2 pi i s_c p_m x_j) exactly as the kernels form it
    (thz_farfield_table); ``p`` [M] host or float64 device values.  C is the number of wavelengths, 1 in frequency
    space."""
    who = "axis_table"
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"{who}: the MI355X path needs a ROCm device (got device {device}); "
                           "this framework has no CPU compute path")
    C = 1 if space == "frequency" else len(torch.as_tensor(wavelengths).reshape(-1))
    p = _vector(p, 1, "frequency", device, who, "p")
    s = _factors(space, wavelengths, C, device, who)
    out = torch.empty(C, p.shape[0], int(n_pix), dtype=torch.complex64, device=device)
    call(_lib.lib().thz_farfield_table, int(n_pix), float(pitch), float(centre), p, 1, p.shape[0], s, C, out, device=device)
    return out


def cut(phi, thetas):
    """Directions of a pattern cut in the plane of azimuth ``phi`` at polar angles ``thetas`` (radians) -> host float64
    [M, 2], (sin theta cos phi, sin theta sin phi)"""
    st = torch.sin(torch.as_tensor(thetas, dtype=torch.float64).reshape(-1))
    return torch.stack([st * math.cos(phi), st * math.sin(phi)], -1)


def uv_grid(half_angle, n):
    """(u, v), host float64 [n] each: direction cosines from -sin(half_angle) to +sin(half_angle) inclusive"""
    e = math.sin(half_angle)
    u = torch.linspace(-e, e, int(n), dtype=torch.float64) if int(n) > 1 else torch.zeros(1, dtype=torch.float64)
    return u, u.clone()
