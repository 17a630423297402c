"""float64 restatement of the measurement kernels (thz_metrics.hip) and of utils/metrics.py in torch ops on
the CPU, pinned on closed forms by tests/test_metrics_cpu.py.

Regions are rows (kind, cr, cc, a, b) with kind "circ" / "rect"; their values are rounded to float32 first (what
the kernel is handed) and every test is made in float64 from those.  ``fp32=True`` runs the same sequence in
float32 (the e32 floor of the backward's bound).  This is also the torch op sequence scripts/metrics_timing.py
times on the device: one mask and one masked pass per region.
"""
import math

import torch


def intensity(x, dtype=torch.float64):
    """I of a field (re^2 + im^2, separate products and one add) or the real input itself."""
    if x.is_complex():
        re, im = x.real.to(dtype), x.imag.to(dtype)
        return re * re + im * im
    return x.to(dtype)


def masks(regions, H, W, device="cpu"):
    """[K + 1, H, W] bool; the last one is the whole plane."""
    i = torch.arange(H, dtype=torch.float64, device=device)[:, None]
    j = torch.arange(W, dtype=torch.float64, device=device)[None, :]
    out = []
    for kind, cr, cc, a, b in regions:
        cr, cc, a, b = (float(torch.tensor(v, dtype=torch.float32)) for v in (cr, cc, a, b))
        di, dj = i - cr, j - cc
        if kind == "circ":
            out.append(di * di + dj * dj <= a * a)
        else:
            out.append((di.abs() <= a) & (dj.abs() <= b))
    out.append(torch.ones(H, W, dtype=torch.bool, device=device))
    return torch.stack([m.expand(H, W) for m in out])


def margin(regions, H, W):
    """The least | |d|^2 - a^2 | (circles) or | |d| - half-size | (rectangles) over every pixel and region: how far
    any membership is from resting on a rounding."""
    i = torch.arange(H, dtype=torch.float64)[:, None]
    j = torch.arange(W, dtype=torch.float64)[None, :]
    least = math.inf
    for kind, cr, cc, a, b in regions:
        cr, cc, a, b = (float(torch.tensor(v, dtype=torch.float32)) for v in (cr, cc, a, b))
        di, dj = i - cr, j - cc
        if kind == "circ":
            least = min(least, float((di * di + dj * dj - a * a).abs().min()))
        else:
            least = min(least, float((di.abs() - a).abs().min()), float((dj.abs() - b).abs().min()))
    return least


def region_sums(x, regions, fp32=False):
    """The five sums [N, K + 1, 5] of [N, H, W], differentiable: S0, Sr, Sc, Srr, Scc."""
    dt = torch.float32 if fp32 else torch.float64
    I = intensity(x, dt)
    N, H, W = I.shape
    m = masks(regions, H, W, I.device)
    i = torch.arange(H, dtype=dt, device=I.device)[:, None].expand(H, W)
    j = torch.arange(W, dtype=dt, device=I.device)[None, :].expand(H, W)
    rows = []
    for k in range(m.shape[0]):
        Im = torch.where(m[k], I, torch.zeros((), dtype=dt, device=I.device))
        rows.append(torch.stack([Im.sum((-2, -1)), (Im * i).sum((-2, -1)), (Im * j).sum((-2, -1)),
                                 (Im * (i * i)).sum((-2, -1)), (Im * (j * j)).sum((-2, -1))], dim=-1))
    return torch.stack(rows, dim=1)


def region_peaks(x, regions):
    """peak [N, K + 1] float64, argmax and count [N, K + 1] int64: the maximum by amax, the argmax as the lowest
    flat index that equals it by explicit comparison; an empty region gives 0, -1, 0."""
    I = intensity(x)
    N, H, W = I.shape
    m = masks(regions, H, W, I.device)
    flat = torch.arange(H * W, device=I.device)
    peak = torch.zeros(N, m.shape[0], dtype=torch.float64, device=I.device)
    arg = torch.full((N, m.shape[0]), -1, dtype=torch.int64, device=I.device)
    cnt = torch.zeros(N, m.shape[0], dtype=torch.int64, device=I.device)
    for k in range(m.shape[0]):
        c = int(m[k].sum())
        cnt[:, k] = c
        if c == 0:
            continue
        Im = torch.where(m[k], I, torch.full((), -math.inf, dtype=torch.float64, device=I.device)).reshape(N, -1)
        pk = Im.amax(dim=-1)
        hit = Im == pk[:, None]
        peak[:, k] = pk
        arg[:, k] = torch.where(hit, flat, torch.full((), H * W, device=I.device)).amin(dim=-1)
    return peak, arg, cnt


def line_widths(v, level, detail=False):
    """[L, 5] float64 = peak, argmax, xl, xr, width of [L, W] lines by a plain loop.  ``detail``: also the
    operands (t, v0, v1) of each crossing, [L, 2, 3], for the tests' bound."""
    v = v.double()
    L, W = v.shape
    out = torch.full((L, 5), math.nan, dtype=torch.float64)
    ops = torch.full((L, 2, 3), math.nan, dtype=torch.float64)
    for l in range(L):
        line = v[l].tolist()
        pk = max(line)
        p = line.index(pk)
        t = level * pk
        out[l, 0], out[l, 1] = pk, p
        for j in range(p - 1, -1, -1):
            if line[j] < t:
                out[l, 2] = j + (t - line[j]) / (line[j + 1] - line[j])
                ops[l, 0] = torch.tensor([t, line[j], line[j + 1]])
                break
        for j in range(p + 1, W):
            if line[j] < t:
                out[l, 3] = j - (t - line[j]) / (line[j - 1] - line[j])
                ops[l, 1] = torch.tensor([t, line[j], line[j - 1]])
                break
        out[l, 4] = out[l, 3] - out[l, 2]
    return (out, ops) if detail else out


# ---- utils/metrics.py ----------------------------------------------------------------------------
def efficiency(x, regions, reference=None):
    s = region_sums(x, regions)[..., 0]
    total = s[:, -1:] if reference is None else region_sums(reference, [])[..., 0]
    return s[:, :-1] / total


def centroid(x, regions, spacing):
    s = region_sums(x, regions)
    mid = torch.tensor([(x.shape[-2] - 1) / 2, (x.shape[-1] - 1) / 2], dtype=torch.float64)
    return (s[..., 1:3] / s[..., 0:1] - mid) * spacing


def d4sigma(x, regions, spacing):
    s = region_sums(x, regions)
    mean = s[..., 1:3] / s[..., 0:1]
    return 4 * torch.sqrt((s[..., 3:5] / s[..., 0:1] - mean * mean).clamp_min(0)) * spacing


def fwhm(x, spacing, level=0.5):
    """[N, 2]: the widths of the column cut and of the row cut through each plane's peak."""
    I = intensity(x)
    _, arg, _ = region_peaks(x, [])
    out = []
    for n in range(I.shape[0]):
        i, j = divmod(int(arg[n, 0]), I.shape[-1])
        out.append(torch.stack([line_widths(I[n, :, j][None], level)[0, 4], line_widths(I[n, i, :][None], level)[0, 4]]))
    return torch.stack(out) * spacing


def interp(z, pos):
    if math.isnan(pos):
        return math.nan
    lo = min(max(int(math.floor(pos)), 0), max(len(z) - 2, 0))
    hi = min(lo + 1, len(z) - 1)
    return z[lo] + (pos - lo) * (z[hi] - z[lo])


def focal_sweep(zx, z_list, spacing, level=0.5, detail=False):
    """peak [Z, M], width [Z, M] (metres), z_left, z_right, depth [M] of a z-x map [Z, M, W]."""
    I = intensity(zx)
    Z, M, W = I.shape
    lw, ops = line_widths(I.reshape(Z * M, W), level, detail=True)
    peak, width = lw[:, 0].reshape(Z, M), lw[:, 4].reshape(Z, M) * spacing
    az = line_widths(peak.t().contiguous(), level)
    z = [float(v) for v in z_list]
    zl = torch.tensor([interp(z, float(p)) for p in az[:, 2]], dtype=torch.float64)
    zr = torch.tensor([interp(z, float(p)) for p in az[:, 3]], dtype=torch.float64)
    res = (peak, width, zl, zr, zr - zl)
    return res + (lw.reshape(Z, M, 5), ops.reshape(Z, M, 2, 3)) if detail else res
