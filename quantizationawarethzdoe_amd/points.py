"""Direct Rayleigh-Sommerfeld propagation to arbitrary detector points -- a module of this port alone like hankel.py,
modes.py and pulse.py (csrc/thz_points.hip).  Every other propagator returns the field on a grid parallel to
the element; a raster-scanned single-pixel detector, a tilted camera, an arc of diffraction orders or a handful of loss
points lie on no such grid.  ``rs_points`` sums the Rayleigh-Sommerfeld integral itself, the kernel function of
RSC_prop / CZT_prop, from every source pixel to every point (the model and the numerical contract are stated in
include/thzdoe.h):

    out[b, c, m] = dx dy sum_ij U[b, c, i, j] G_c(x_m - x_j, y_m - y_i, z_m)

at O(M H W) per channel and batch entry, with no aliasing window, no padding and no restriction on the points.  The kernel
matrix is generated in registers (fp64 geometry and phase reduction, fp32 amplitude and sums) and never stored.

Pixel (i, j) of a field of pitch (dx, dy) is at x = x0 + (j - (W - 1) / 2) dx, y = y0 + (i - (H - 1) / 2) dy with
``origin`` = (x0, y0): dim -1 is x, dim -2 is y.  A ``[3, C, H, W]`` vectorial field's components ride the batch axis.

Host points (a list, numpy, a CPU tensor) are checked -- finite, z > 0 -- and uploaded, a blocking copy; a device tensor
is converted to float64 and taken as it is, unchecked (a z <= 0 there gives a non-finite or meaningless sum), with no
sync, so the call is capturable in torch.cuda.graph.  A repeated call gives the same bits, and B entries in one call the
bits of the entries one at a time at the same ``chunks``.
"""
import math

import torch

from . import _lib
from ._call import _fptr, _require_device, call, workspace


def _floats(v):
    return [float(x) for x in (v.reshape(-1).tolist() if torch.is_tensor(v) else v if isinstance(v, (list, tuple)) else [v])]


def _pair(v, who, what):
    v = _floats(v)
    if len(v) == 1:
        v = v * 2
    if len(v) != 2:
        raise ValueError(f"{who}: {what} is a scalar or a pair; got {v}")
    return tuple(v)


def host_points(points, who="rs_points"):
    """``points`` [..., 3] (a list, numpy or a CPU tensor, metres) as a checked float64 CPU tensor: finite, z > 0"""
    p = torch.as_tensor(points).detach().to("cpu", torch.float64)
    if p.dim() < 1 or p.shape[-1] != 3 or p.numel() == 0:
        raise ValueError(f"{who}: points are [..., 3] (x, y, z); got {tuple(p.shape)}")
    if not bool(torch.isfinite(p).all()):
        raise ValueError(f"{who}: the points must be finite")
    if not bool((p[..., 2] > 0).all()):
        raise ValueError(f"{who}: every point needs z > 0 (the field is on the plane z = 0); "
                         f"got min z = {float(p[..., 2].min())}")
    return p


def scan_line(start, stop, n):
    """``n`` points from ``start`` to ``stop`` (both (x, y, z), inclusive) -> host float64 [n, 3]: the path of a
    raster-scanned single-pixel detector"""
    a, b = (torch.as_tensor(v, dtype=torch.float64).reshape(3) for v in (start, stop))
    s = torch.linspace(0.0, 1.0, int(n), dtype=torch.float64)[:, None] if int(n) > 1 else torch.zeros(1, 1, dtype=torch.float64)
    return a[None, :] + s * (b - a)[None, :]


def tilted_plane(shape, pitch, center, tilt_x=0.0, tilt_y=0.0):
    """A detector grid of ``shape`` = (H', W') pixels of ``pitch`` (a scalar or (px, py)) about ``center`` = (x, y, z),
    rotated about its centre by ``tilt_x`` then ``tilt_y`` (radians, about the x and the y axis) -> host float64
    [H', W', 3].  Zero tilt is the flat grid u = (j - (W' - 1) / 2) px, v = (i - (H' - 1) / 2) py at z = center[2];
    a rotation keeps the pitch."""
    Hp, Wp = (int(v) for v in shape)
    px, py = _pair(pitch, "tilted_plane", "pitch")
    c = torch.as_tensor(center, dtype=torch.float64).reshape(3)
    u = (torch.arange(Wp, dtype=torch.float64) - (Wp - 1) / 2) * px
    v = (torch.arange(Hp, dtype=torch.float64) - (Hp - 1) / 2) * py
    local = torch.stack([u[None, :].expand(Hp, Wp), v[:, None].expand(Hp, Wp), torch.zeros(Hp, Wp, dtype=torch.float64)], -1)
    cx, sx, cy, sy = math.cos(tilt_x), math.sin(tilt_x), math.cos(tilt_y), math.sin(tilt_y)
    Rx = torch.tensor([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], dtype=torch.float64)
    Ry = torch.tensor([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=torch.float64)
    return local @ (Ry @ Rx).T + c


def _desc(shape, M, cfg):
    B, C, H, W = shape
    wl, (dx, dy), (x0, y0), chunks = cfg
    arr = _lib.float_array(wl)
    d = _lib.PointsDesc(B=B, C=C, H=H, W=W, M=M, chunks=chunks, dx=dx, dy=dy, x0=x0, y0=y0, wavelengths=_fptr(arr))
    d._keep = arr
    return d


class _Forward(torch.autograd.Function):
    """out [B, C, M] of thz_rs_points_forward; the sum is linear, so the backward is thz_rs_points_adjoint."""

    @staticmethod
    def forward(ctx, field, pts, cfg):
        ctx.pts, ctx.cfg, ctx.shape = pts, cfg, tuple(field.shape)
        B, C = field.shape[:2]
        d = _desc(field.shape, pts.shape[0], cfg)
        out = torch.empty(B, C, pts.shape[0], dtype=torch.complex64, device=field.device)
        ws = workspace(_lib.lib().thz_rs_points_workspace_size, d, device=field.device)
        call(_lib.lib().thz_rs_points_forward, d, field.contiguous(), pts, out, ws, ws.numel(), device=field.device)
        return out

    @staticmethod
    def backward(ctx, g):
        return _Adjoint.apply(g.resolve_conj(), ctx.pts, ctx.cfg, ctx.shape), None, None


class _Adjoint(torch.autograd.Function):
    """grad_field [B, C, H, W] of thz_rs_points_adjoint; its backward is thz_rs_points_forward."""

    @staticmethod
    def forward(ctx, g, pts, cfg, shape):
        ctx.pts, ctx.cfg = pts, cfg
        out = torch.empty(shape, dtype=torch.complex64, device=g.device)
        call(_lib.lib().thz_rs_points_adjoint, _desc(shape, pts.shape[0], cfg), g.contiguous(), pts, out, device=g.device)
        return out

    @staticmethod
    def backward(ctx, g):
        return _Forward.apply(g.resolve_conj(), ctx.pts, ctx.cfg), None, None, None


def rs_points(field, points, wavelengths=None, spacing=None, origin=(0.0, 0.0), chunks=None):
    """The field at arbitrary points: ``field`` an ElectricField (data, wavelengths and spacing) or a complex64
    [B, C, H, W] tensor with ``wavelengths=`` and ``spacing=`` (a scalar or (dx, dy)) -> complex64
    [B, C, *points.shape[:-1]] (thz_rs_points_forward).  ``points`` [..., 3] in metres, on the host (checked and
    uploaded) or on the device (converted to float64, taken as it is); ``origin`` is the (x, y) of the field's centre.
    ``chunks`` fixes how many ranges the forward cuts the pixels into (clamped to 1 .. ceil(H W / 256)); None is the
    library's choice, a function of the shape alone.  Gradients flow to the field (thz_rs_points_adjoint), none to the
    points."""
    who = "rs_points"
    if not torch.is_tensor(field) and hasattr(field, "data"):
        wavelengths = field.wavelengths_host if wavelengths is None else wavelengths
        spacing = field.spacing_host if spacing is None else spacing
        field = field.data
    if not torch.is_tensor(field):
        raise TypeError(f"{who}: the field must be a tensor or an ElectricField")
    if field.dtype == torch.complex128:
        raise TypeError(f"{who}: the kernels compute in complex64; got a complex128 field -- cast it, an fp64 "
                        "variant does not exist")
    if field.dtype != torch.complex64 or field.dim() != 4:
        raise TypeError(f"{who}: the field is complex64 [B, C, H, W]; got {field.dtype} {tuple(field.shape)}")
    if wavelengths is None or spacing is None:
        raise ValueError(f"{who}: a tensor needs wavelengths= and spacing=")
    if not (torch.is_tensor(points) and points.is_cuda):
        points = host_points(points, who)
    elif points.dim() < 1 or points.shape[-1] != 3 or points.numel() == 0:
        raise ValueError(f"{who}: points are [..., 3] (x, y, z); got {tuple(points.shape)}")
    _require_device(field, who)
    wl = tuple(_floats(wavelengths))
    if len(wl) != field.shape[1]:
        raise ValueError(f"{who}: {len(wl)} wavelengths for a field of {field.shape[1]} channels")
    cfg = (wl, _pair(spacing, who, "spacing"), _pair(origin, who, "origin"), 0 if chunks is None else max(1, int(chunks)))
    lead = tuple(points.shape[:-1])
    pts = points.detach().to(field.device, torch.float64).reshape(-1, 3).contiguous()
    return _Forward.apply(field.resolve_conj(), pts, cfg).reshape(*field.shape[:2], *lead)
