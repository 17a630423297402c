"""The measurement kernels behind utils/metrics.py: region statistics and line widths (csrc/thz_metrics.hip;
DESIGN §29).
"""
import collections
import ctypes
import math

import torch

from .. import _lib
from .._call import _require_device, call, workspace
from .heightmap import as_planes

RegionStats = collections.namedtuple("RegionStats", "power moment1 moment2 peak argmax count")
LineWidths = collections.namedtuple("LineWidths", "peak argmax left right width")

_METRICS_DTYPES = {torch.complex64: _lib.METRICS_C64, torch.complex128: _lib.METRICS_C128,
                   torch.float32: _lib.METRICS_F32, torch.float64: _lib.METRICS_F64}
_REGION_KINDS = {"circ": _lib.REGION_CIRC, "rect": _lib.REGION_RECT}


def region_table(regions, kind, who, device):
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
        ws = workspace(_lib.lib().thz_region_stats_workspace_size, d, device=x.device)
        call(_lib.lib().thz_region_stats_forward, d, x, out, ws, ws.numel(), device=x.device)
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
        call(_lib.lib().thz_region_stats_backward, d, x, G, grad, device=x.device)
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
    p = as_planes(x.resolve_conj().contiguous(), who)
    table = region_table(regions, kind, who, x.device)
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
    call(_lib.lib().thz_line_widths, v, _METRICS_DTYPES[v.dtype], out.shape[0], W, level, out, device=v.device)
    out = out.reshape(tuple(v.shape[:-1]) + (5,))
    return LineWidths(out[..., 0], out[..., 1].to(torch.int64), out[..., 2], out[..., 3], out[..., 4])
