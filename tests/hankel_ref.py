"""The Hankel propagator's model (include/thzdoe.h) in torch on tables that are handed in, and an independent fp64
builder of the table from scipy.special.  Plain helper module: no test, no fixture.
"""
import numpy as np
import torch


def forward(T, w, H, f, keep, cdtype=torch.complex128):
    """out [Z, B, C, keep] from T [N, N], w [N], H [Z, C, N], f [B, C, N], everything at ``cdtype`` with torch's CPU
    matmul; differentiable in ``f``."""
    rdtype = torch.float64 if cdtype == torch.complex128 else torch.float32
    Tc, w, H = T.to(cdtype), w.to(rdtype), H.to(cdtype)
    F = (w * f.to(cdtype)) @ Tc.T                       # F[b, c, m] = sum_n T[m, n] w_n f[b, c, n]
    return ((H[:, None] * F[None]) @ Tc[:keep].T) / w[:keep]


def transfer(zeros, r_max, wavelengths, z_list):
    """H complex128 [Z, C, N] by the header's fp64 formula, operation by operation; wavelengths and z are the float32
    values the kernels receive."""
    lam = torch.tensor(wavelengths, dtype=torch.float32).double()
    z = torch.tensor(z_list, dtype=torch.float32).double()
    k = (6.283185307179586 / lam)[None, :, None]
    kap = (zeros[:-1].double() / r_max)[None, None, :]
    live = kap < k
    ph = z[:, None, None] * torch.sqrt(torch.where(live, k * k - kap * kap, torch.zeros_like(kap)))
    return torch.where(live, torch.polar(torch.ones_like(ph), ph), torch.zeros_like(ph, dtype=torch.complex128))


def table_at(zeros):
    """(T, w) float64 of the model at the zeros j_1 .. j_{N+1} (numpy float64), J0 and J1 from scipy"""
    from scipy import special
    j, S = zeros[:-1], zeros[-1]
    a = np.abs(special.j1(j))
    return 2.0 * special.j0(np.outer(j, j) / S) / (np.outer(a, a) * S), 1.0 / a


def scipy_table(N):
    """(T, w, zeros) float64, the zeros from scipy.special.jn_zeros"""
    from scipy import special
    zeros = special.jn_zeros(0, N + 1)
    return table_at(zeros) + (zeros,)
