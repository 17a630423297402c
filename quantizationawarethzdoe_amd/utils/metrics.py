"""Focal-spot figures of merit on the measurement kernels of csrc/thz_metrics.hip.

The reference's ``utils/metrics.py`` is an empty placeholder; its notebooks judge a design by eye.  These
functions grade one: the power in each spot, the uniformity of the spots, their centroids and widths, and
the depth over which a focus holds.  Each makes one pass over the field (``optics.region_stats``) or over a
set of lines (``optics.line_widths``) and finishes in float64 torch arithmetic on the few numbers that come
back; nothing reads the device, so every function can run inside a captured step.  Efficiency, centroid and
D4-sigma are differentiable in the field.

``field`` is an ``ElectricField``, a complex tensor (I = |E|^2) or a real intensity tensor, the two spatial
dimensions last; regions are rows (cr, cc, a) / (cr, cc, a, b) in pixel units as ``optics.region_stats``
takes them (``spot_regions`` makes them from the notebooks' metre positions).  Results carry the leading
dimensions of the field, then the regions.
"""
import collections

import torch

from .. import optics

FocalSweep = collections.namedtuple("FocalSweep", "peak width z_left z_right depth_of_focus")


def _data(field):
    return field.data if hasattr(field, "data") and not torch.is_tensor(field) else field


def _scaled(t, spacing, offset=(0.0, 0.0)):
    """(t[..., 0] - offset[0]) dy, (t[..., 1] - offset[1]) dx for a pitch given as a scalar or (dy, dx).  Host
    numbers stay host numbers (no copy to the device); a device tensor is used where it is."""
    if torch.is_tensor(spacing) and spacing.is_cuda:
        s = spacing.detach().double().reshape(-1)
        dy, dx = (s[0], s[0]) if s.numel() == 1 else (s[0], s[1])
    else:
        s = [float(v) for v in torch.as_tensor(spacing).reshape(-1)]
        if len(s) not in (1, 2):
            raise ValueError(f"spacing must be a scalar or (dy, dx); got {spacing!r}")
        dy, dx = s[0], s[-1]
    return torch.stack(((t[..., 0] - offset[0]) * dy, (t[..., 1] - offset[1]) * dx), dim=-1)


def spot_regions(resolution, sampling_size, positions, radius):
    """Circular regions [K, 3] (cr, cc, a) in pixels for spots at ``positions`` (metres) of ``radius`` (metres)
    on the grid of ``qat.define_FoM(resolution, sampling_size, ...)``, quirks included: with
    ``height, width = resolution`` its axis along dim -2 is ``linspace(-Lx / 2, Lx / 2, width)`` with
    ``Lx = sampling_size * width`` and takes ``position[0]``; dim -1 is ``linspace(-Ly / 2, Ly / 2, height)`` and
    takes ``position[1]``.  The pixel pitch is therefore L / (n - 1), not ``sampling_size``.  The radius is
    converted with the pitch of dim -2; the two pitches must agree (a square grid) for the circle to be one."""
    height, width = int(resolution[0]), int(resolution[1])
    if height < 2 or width < 2:
        raise ValueError(f"spot_regions: the grid needs two points per axis; got resolution {resolution!r}")
    Lx, Ly = float(sampling_size) * width, float(sampling_size) * height
    pr, pc = Lx / (width - 1), Ly / (height - 1)
    if abs(pr - pc) > 1e-9 * max(pr, pc):
        raise ValueError(f"spot_regions: pitches {pr} and {pc} differ; circles need a square grid")
    rows = [[(float(p[0]) + Lx / 2) / pr, (float(p[1]) + Ly / 2) / pc, float(radius) / pr] for p in positions]
    return torch.tensor(rows, dtype=torch.float64).reshape(-1, 3)


def diffraction_efficiency(field, regions, reference=None, kind="circ"):
    """Power in each region over the power of the whole plane, [..., K]; with ``reference`` (the field before
    the DOE) over the whole-plane power of ``reference`` instead."""
    power = optics.region_stats(_data(field), regions, kind).power
    total = power[..., -1:] if reference is None else optics.region_stats(_data(reference), [], "circ").power
    return power[..., :-1] / total


def spot_uniformity(powers):
    """(max - min) / (max + min) over the last dimension: of region powers or of region peaks."""
    hi, lo = powers.amax(dim=-1), powers.amin(dim=-1)
    return (hi - lo) / (hi + lo)


def centroid(field, regions, spacing, kind="circ"):
    """Intensity centroid of every region and of the whole plane (last), [..., K + 1, 2] = (y, x) in metres
    from the plane's centre pixel ((H - 1) / 2, (W - 1) / 2); ``spacing`` is the pixel pitch, a scalar or
    (dy, dx)."""
    x = _data(field)
    st = optics.region_stats(x, regions, kind)
    return _scaled(st.moment1 / st.power[..., None], spacing, ((x.shape[-2] - 1) / 2, (x.shape[-1] - 1) / 2))


def d4sigma(field, regions, spacing, kind="circ"):
    """D4-sigma widths 4 sqrt(<u^2> - <u>^2) of every region and of the whole plane (last), [..., K + 1, 2] =
    (along y, along x) in metres."""
    x = _data(field)
    st = optics.region_stats(x, regions, kind)
    mean = st.moment1 / st.power[..., None]
    var = st.moment2 / st.power[..., None] - mean * mean
    return _scaled(4 * torch.sqrt(var.clamp_min(0)), spacing)


def encircled_energy(field, center, radii):
    """Power inside concentric circles of ``radii`` (pixels, up to 16) about ``center`` = (row, column) in
    pixels, over the whole-plane power, [..., len(radii)]; one kernel call."""
    regions = [[float(center[0]), float(center[1]), float(r)] for r in radii]
    return diffraction_efficiency(field, regions)


def _intensity(lines):
    """|E|^2 in float64 (exact products for a complex64 field); a real input is the intensity already."""
    if not lines.is_complex():
        return lines
    re, im = lines.real.double(), lines.imag.double()
    return re * re + im * im


def fwhm(field, spacing, level=0.5):
    """Width at ``level`` x peak of the column cut and of the row cut through each plane's peak, [..., 2] =
    (along y, along x) in metres; NaN where a cut does not fall below the level before the edge.  The two
    lines are gathered by the device-side argmax: no host read."""
    x = _data(field)
    H, W = x.shape[-2], x.shape[-1]
    arg = optics.region_stats(x.detach(), [], "circ").argmax[..., 0].reshape(-1)
    planes = x.detach().reshape(-1, H, W)
    n = torch.arange(planes.shape[0], device=x.device)
    i, j = torch.div(arg, W, rounding_mode="floor"), arg % W
    cuts = (_intensity(planes[n, :, j]), _intensity(planes[n, i, :]))  # along y [N, H], along x [N, W]
    widths = _scaled(torch.stack([optics.line_widths(c.contiguous(), level).width for c in cuts], dim=-1), spacing)
    return widths.reshape(tuple(x.shape[:-2]) + (2,))


def _interp(z, pos):
    """z at fractional index ``pos`` by linear interpolation of the 1-D ``z``; NaN stays NaN."""
    bad = torch.isnan(pos)
    q = torch.where(bad, torch.zeros_like(pos), pos)
    lo = q.floor().clamp(0, max(z.numel() - 2, 0)).long()
    hi = (lo + 1).clamp(max=z.numel() - 1)
    out = z[lo] + (q - lo) * (z[hi] - z[lo])
    return torch.where(bad, pos, out)


def focal_sweep(zx, z_list, spacing, level=0.5):
    """Peak and width against z of a z-x map [Z, ..., W] (any ``propagate_zx``; complex or intensity), and the
    depth of focus.  Returns ``FocalSweep``: ``peak`` [Z, ...] and ``width`` [Z, ...] (metres, ``spacing`` the
    pitch along the line) of every z-line; ``z_left``, ``z_right`` and ``depth_of_focus`` [...]: the width at
    ``level`` of the peak-against-z line, its crossings mapped to z by linear interpolation of ``z_list`` (so a
    non-uniform sweep is measured in metres, not in planes).  NaN where the focus does not fall below the
    level inside the sweep."""
    x = _data(zx).detach()
    z = torch.as_tensor(z_list, dtype=torch.float64).reshape(-1).to(x.device)
    if x.dim() < 2 or x.shape[0] != z.numel():
        raise ValueError(f"focal_sweep: the map {tuple(x.shape)} needs one leading entry per z ({z.numel()})")
    lw = optics.line_widths(_intensity(x).contiguous(), level)
    along_z = optics.line_widths(lw.peak.movedim(0, -1).contiguous(), level)
    zl, zr = _interp(z, along_z.left), _interp(z, along_z.right)
    return FocalSweep(lw.peak, lw.width * float(spacing), zl, zr, zr - zl)
