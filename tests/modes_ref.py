"""The Hermite-Gauss model (include/thzdoe.h: thz_hg_*) restated in torch: the recurrence in fp64 and the two products on
tables that are handed in.  Plain helper module: no test, no fixture.
"""
import math

import torch


def table(n_modes, n_pix, pitch, waists, centre):
    """G float64 [C, n_modes, n_pix]: u_k(x_j) = sqrt(sqrt(2) / w) psi_k(sqrt(2) x_j / w) at
    x_j = (j - (n_pix - 1) / 2) pitch - centre, by the three-term recurrence"""
    w = torch.tensor([float(v) for v in waists], dtype=torch.float64)[:, None]
    x = (torch.arange(n_pix, dtype=torch.float64) - (n_pix - 1) / 2) * pitch - centre
    xi = math.sqrt(2.0) * x[None, :] / w
    rows = [math.pi ** -0.25 * torch.exp(-xi * xi / 2)]
    prev = torch.zeros_like(xi)
    for k in range(n_modes - 1):
        rows.append(math.sqrt(2.0 / (k + 1)) * xi * rows[-1] - math.sqrt(k / (k + 1)) * prev)
        prev = rows[-2]
    return torch.sqrt(math.sqrt(2.0) / w)[:, None] * torch.stack(rows, dim=1)


def decompose(Gy, U, Gx, scale, cdtype=torch.complex128):
    """c [B, C, M, N] = scale sum_ij Gy[c, m, i] U[b, c, i, j] Gx[c, n, j] at ``cdtype``; differentiable in U"""
    return scale * torch.einsum("cmi,bcij,cnj->bcmn", Gy.to(cdtype), U.to(cdtype), Gx.to(cdtype))


def synthesize(Gy, c, Gx, scale, cdtype=torch.complex128):
    """U [B, C, H, W] = scale sum_mn Gy[c, m, i] c[b, c, m, n] Gx[c, n, j] at ``cdtype``; differentiable in c"""
    return scale * torch.einsum("cmi,bcmn,cnj->bcij", Gy.to(cdtype), c.to(cdtype), Gx.to(cdtype))
