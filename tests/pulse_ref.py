"""The pulse model (include/thzdoe.h: thz_pulse_*) restated in torch on a table that is handed in.  Plain helper module:
no test, no fixture.
"""
import torch

C64, C128 = torch.complex64, torch.complex128


def synthesize(table, U, cdtype=C128):
    """E [B, T, H, W] = sum_c table[j, c] U[b, c, h, w] at ``cdtype``; differentiable in U"""
    return torch.einsum("jc,bchw->bjhw", table.to(cdtype), U.to(cdtype))


def adjoint(table, g, cdtype=C128):
    """Ubar [B, C, H, W] = sum_j conj(table[j, c]) g[b, j, h, w] at ``cdtype``"""
    return torch.einsum("jc,bjhw->bchw", table.to(cdtype).conj(), g.to(cdtype))


def maps(table, times, dt, U, dtype=torch.float64):
    """(energy, peak, t_peak, t_mean, t_rms) stacked to [B, 5, H, W] at ``dtype``, with j* [B, H, W] beside it;
    differentiable in U (a dark pixel's t_mean and t_rms are constants)"""
    E = synthesize(table, U, C128 if dtype == torch.float64 else C64)
    I = E.real ** 2 + E.imag ** 2
    t, w = times.to(dtype)[None, :, None, None], dt.to(dtype)[None, :, None, None]
    W = (I * w).sum(1)
    peak = I.amax(1).detach()
    idx = torch.arange(I.shape[1])[None, :, None, None]
    j = torch.where(I.detach() == peak[:, None], idx, I.shape[1]).amin(1)   # the smallest j that reaches the peak
    lit = W > 0
    Ws = torch.where(lit, W, torch.ones_like(W))
    t_mean = torch.where(lit, (t * I * w).sum(1) / Ws, torch.zeros_like(W))
    var = torch.where(lit, ((t - t_mean[:, None]) ** 2 * I * w).sum(1) / Ws, torch.zeros_like(W))
    t_rms = torch.where(var > 0, torch.sqrt(torch.where(var > 0, var, torch.ones_like(var))), torch.zeros_like(var))
    return torch.stack([W, I.gather(1, j[:, None])[:, 0], times.to(dtype)[j], t_mean, t_rms], 1), j
