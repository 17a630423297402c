"""The direct Rayleigh-Sommerfeld sum to points (include/thzdoe.h: thz_rs_points_*) restated with torch on the CPU.

``float64`` is the sum in complex128.  ``float32`` is the numerical contract's algebra: geometry and frac(r / lambda) in
fp64, the fraction rounded to fp32, then sine / cosine, amplitude, products and sums in fp32 / complex64.

Plain helper module: no test, no fixture.
"""
import math

import torch


def kernel(points, H, W, lam, spacing, origin=(0.0, 0.0), dtype=torch.float64):
    """dx dy G_c(x_m - x_j, y_m - y_i, z_m) -> [C, M, H, W]; ``points`` [M, 3] and ``lam`` [C] float64"""
    dx, dy = spacing
    x = origin[0] + (torch.arange(W, dtype=torch.float64) - (W - 1) / 2) * dx
    y = origin[1] + (torch.arange(H, dtype=torch.float64) - (H - 1) / 2) * dy
    X = points[:, 0, None, None] - x[None, None, :]
    Y = points[:, 1, None, None] - y[None, :, None]
    z = points[:, 2, None, None].expand(-1, H, W)
    r = torch.sqrt(X ** 2 + Y ** 2 + z ** 2)
    lam = lam.double()[:, None, None, None]
    if dtype == torch.float64:
        k = 2 * math.pi / lam
        return torch.exp(1j * k * r) * (z / (2 * math.pi * r ** 2) * (dx * dy)) * (1 / r - 1j * k)
    t = r / lam
    ang = (2 * math.pi) * (t - torch.floor(t)).float()
    rf, zf, kf = r.float(), z.float(), (2 * math.pi / lam).float()
    amp = zf / (2 * math.pi * rf ** 2) * (dx * dy)
    return torch.complex(torch.cos(ang), torch.sin(ang)) * torch.complex((amp / rf).expand_as(ang), -(amp * kf))


def rs_points(U, points, lam, spacing, origin=(0.0, 0.0), dtype=torch.float64):
    """out[b, c, m] = dx dy sum_ij U[b, c, i, j] G_c(...); ``U`` [B, C, H, W]"""
    G = kernel(points, U.shape[-2], U.shape[-1], lam, spacing, origin, dtype)
    return torch.einsum("bchw,cmhw->bcm", U.to(G.dtype), G)


def adjoint(g, points, lam, spacing, shape, origin=(0.0, 0.0), dtype=torch.float64):
    """grad[b, c, i, j] = dx dy sum_m conj(G_c(...)) g[b, c, m]; ``g`` [B, C, M], ``shape`` = (H, W)"""
    G = kernel(points, shape[0], shape[1], lam, spacing, origin, dtype)
    return torch.einsum("bcm,cmhw->bchw", g.to(G.dtype), G.conj())
