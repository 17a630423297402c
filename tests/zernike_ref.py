"""Restatements of the Zernike model of include/thzdoe.h (thz_zernike_*) on the CPU: the closed form in fp64, the
header's recurrence in a given dtype, and the products and the least-squares solve as einsum in a given dtype.

Plain helper module: no test, no fixture.
"""
import math

import torch

F64 = torch.float64


def orders(n_max):
    """[(n, m)] in OSA / ANSI order, k = (n (n + 2) + m) / 2"""
    return [(n, m) for n in range(n_max + 1) for m in range(-n, n + 1, 2)]


def norm(n, m):
    return math.sqrt(n + 1 if m == 0 else 2 * (n + 1))


def geometry(shape, spacing, pupil):
    """fp64 (x [H, W], y [H, W], inside [H, W]) in the header's operation order"""
    (H, W), (dx, dy), (x0, y0, R) = shape, spacing, pupil
    x = ((torch.arange(W, dtype=F64) - (W - 1) / 2) * dx - x0)[None, :].expand(H, W)
    y = ((torch.arange(H, dtype=F64) - (H - 1) / 2) * dy - y0)[:, None].expand(H, W)
    return x, y, x * x + y * y <= R * R


def closed_form(shape, spacing, pupil, n_max):
    """Z fp64 [K, H, W]: the explicit sum with exact integer coefficients (good to ~1e-11 at n = 14 in fp64)"""
    x, y, inside = geometry(shape, spacing, pupil)
    rho, theta = torch.sqrt(x * x + y * y) / pupil[2], torch.atan2(y, x)
    out = []
    for n, m in orders(n_max):
        a = abs(m)
        rad = sum((-1) ** k * (math.factorial(n - k) // (math.factorial(k) * math.factorial((n + a) // 2 - k)
                                                         * math.factorial((n - a) // 2 - k))) * rho ** (n - 2 * k)
                  for k in range((n - a) // 2 + 1))
        out.append(norm(n, m) * rad * (torch.cos(a * theta) if m >= 0 else torch.sin(a * theta)) * inside)
    return torch.stack(out)


def recurrence(shape, spacing, pupil, n_max, dtype):
    """Z [K, H, W] by the header's recurrences carried in ``dtype``: geometry in fp64 rounded once, coefficients
    formed in fp64 and rounded once, plain multiplies and adds where the kernel fuses"""
    x, y, inside = geometry(shape, spacing, pupil)
    r = torch.sqrt(x * x + y * y)
    rho64 = r / pupil[2]
    safe = torch.where(r > 0, r, torch.ones_like(r))
    ct, st = torch.where(r > 0, x / safe, torch.ones_like(r)).to(dtype), (y / safe).to(dtype)
    rho, t = rho64.to(dtype), (2 * rho64 * rho64 - 1).to(dtype)
    Z = {}
    pm, cm, sm, cm1, sm1 = inside.to(dtype), torch.ones_like(ct), torch.zeros_like(ct), None, None
    for m in range(n_max + 1):
        prev, cur = torch.zeros_like(pm), pm
        for s in range((n_max - m) // 2 + 1):
            n, c = m + 2 * s, 2 * s + m
            if s == 1:
                cur, prev = ((m + 2) / 2 * t - m / 2) * cur, cur
            elif s > 1:
                D = 2 * s * (s + m) * (c - 2)
                A, B, C = (c - 1) * c * (c - 2) / D, (c - 1) * m * m / D, 2 * (s - 1) * (s + m - 1) * c / D
                cur, prev = (A * t - B) * cur - C * prev, cur
            v = norm(n, m) * cur
            Z[n, m] = v * cm
            if m:
                Z[n, -m] = v * sm
        if m == 0:
            cm1, sm1, cm, sm = cm, sm, ct, st
        else:
            cm1, sm1, cm, sm = cm, sm, 2 * ct * cm - cm1, 2 * ct * sm - sm1
        pm = pm * rho
    return torch.stack([Z[nm] for nm in orders(n_max)])


def project(Z, w, dtype=F64):
    return torch.einsum("khw,bhw->bk", Z.to(dtype), w.to(dtype))


def gram(Z, dtype=F64):
    return torch.einsum("khw,lhw->kl", Z.to(dtype), Z.to(dtype))


def synthesize(Z, a, dtype=F64):
    return torch.einsum("bk,khw->bhw", a.to(dtype), Z.to(dtype))


def solve(Z, w, dtype=F64):
    """the least-squares coefficients [B, K]: G a = S in ``dtype``"""
    return torch.linalg.solve(gram(Z, dtype), project(Z, w, dtype).T).T
