"""The far-field model (include/thzdoe.h: thz_farfield_*) restated in torch: one axis' table by the closed form in fp64
and by the numerical contract in fp32, and the list and grid products as einsums on tables that are handed in.  Plain
helper module: no test, no fixture.
"""
import math

import torch

C64, C128 = torch.complex64, torch.complex128


def table(n_pix, pitch, centre, p, s, dtype=torch.float64):
    """E [C, M, n_pix] = exp(-2 pi i x_j s_c p_m) at x_j = (j - (n_pix - 1) / 2) pitch - centre; ``p`` [M] and ``s`` [C]
    float64.  float64: the closed form in complex128.  float32: the contract -- coordinate, frequency, the phase in
    turns and its reduction in fp64, rounded once, cosine and sine in fp32 -- in complex64."""
    x = (-0.5 * (n_pix - 1) * pitch - centre) + torch.arange(n_pix, dtype=torch.float64) * pitch
    t = x[None, None, :] * (s.double()[:, None] * p.double()[None, :])[:, :, None]
    if dtype == torch.float64:
        return torch.exp(-2j * math.pi * t)
    ang = (2 * math.pi) * (t - torch.round(t)).float()
    return torch.complex(torch.cos(ang), -torch.sin(ang))


def oblique(p, q, s, cdtype=C128):
    """-i w s_c with w = sqrt(max(0, 1 - p^2 - q^2)), broadcast over p and q -> [C, *p.shape]"""
    w = torch.sqrt(torch.clamp(1 - p.double() ** 2 - q.double() ** 2, min=0))
    return (-1j * s.double().reshape(-1, *[1] * w.dim()) * w).to(cdtype)


def list_forward(Ey, U, Ex, scale, fac=None, cdtype=C128):
    """A [B, C, M] = scale fac[c, m] sum_ij U[b, c, i, j] Ex[c, m, j] Ey[c, m, i] at ``cdtype``; differentiable in U"""
    out = scale * torch.einsum("bcij,cmj,cmi->bcm", U.to(cdtype), Ex.to(cdtype), Ey.to(cdtype))
    return out if fac is None else out * fac.to(cdtype)


def list_adjoint(Ey, g, Ex, scale, fac=None, cdtype=C128):
    """G [B, C, H, W] = scale sum_m conj(fac Ex Ey) g[b, c, m]"""
    g = g.to(cdtype) if fac is None else g.to(cdtype) * fac.to(cdtype).conj()
    return scale * torch.einsum("bcm,cmj,cmi->bcij", g, Ex.to(cdtype).conj(), Ey.to(cdtype).conj())


def grid_forward(Ey, U, Ex, scale, fac=None, cdtype=C128):
    """A [B, C, Mv, Mu] = scale fac[c, v, u] sum_ij U[b, c, i, j] Ex[c, u, j] Ey[c, v, i]; differentiable in U"""
    out = scale * torch.einsum("bcij,cuj,cvi->bcvu", U.to(cdtype), Ex.to(cdtype), Ey.to(cdtype))
    return out if fac is None else out * fac.to(cdtype)


def grid_adjoint(Ey, g, Ex, scale, fac=None, cdtype=C128):
    """G [B, C, H, W] = scale sum_vu conj(fac Ex Ey) g[b, c, v, u]"""
    g = g.to(cdtype) if fac is None else g.to(cdtype) * fac.to(cdtype).conj()
    return scale * torch.einsum("bcvu,cuj,cvi->bcij", g, Ex.to(cdtype).conj(), Ey.to(cdtype).conj())


def orders(U, mx, my, dtype=torch.float64, period=None):
    """eta [B, C, len(my), len(mx)] = |1 / (H W) sum U exp(-2 pi i (m x / Lx + n y / Ly))|^2 at unit pitch and the
    period (Lx, Ly) in pixels (None: the extent); the tables by ``table`` at ``dtype``"""
    H, W = U.shape[-2:]
    Lx, Ly = (W, H) if period is None else period
    one = torch.ones(1, dtype=torch.float64)
    Ex = table(W, 1.0, 0.0, torch.tensor([m / Lx for m in mx], dtype=torch.float64), one, dtype)
    Ey = table(H, 1.0, 0.0, torch.tensor([n / Ly for n in my], dtype=torch.float64), one, dtype)
    cdtype = C128 if dtype == torch.float64 else C64
    a = grid_forward(Ey.expand(U.shape[1], -1, -1), U, Ex.expand(U.shape[1], -1, -1), 1.0 / (H * W), None, cdtype)
    return a.real ** 2 + a.imag ** 2
