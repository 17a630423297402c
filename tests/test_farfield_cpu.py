"""The far-field restatement (tests/farfield_ref.py) pinned to closed forms, in fp64 on the CPU."""
import math

import torch

from tests import farfield_ref as ref
from tests import gpu_util, points_ref


def test_grating_orders():
    """a 0 / pi grating of period 8 and duty 1 / 2: the order amplitudes are the DFT of the cell, a_m = 1 / 8 sum_j
    U_j exp(-2 pi i m x_j / 8): eta = 0 at even m, |sin(pi m / 2) / (4 sin(pi m / 8))|^2 at odd m"""
    j = torch.arange(64)
    U = torch.exp(1j * math.pi * ((j % 8) < 4).double()).expand(1, 1, 16, 64)
    ms = tuple(range(-3, 4))
    eta = ref.orders(U, ms, (0,), torch.float64, (8, 16))[0, 0, 0]
    want = torch.tensor([0.0 if m % 2 == 0 else (1 / (4 * math.sin(math.pi * m / 8))) ** 2 for m in ms], dtype=torch.float64)
    assert float((eta - want).abs().max()) <= 1e-14


def test_parseval():
    """the efficiencies of all H W orders of the extent sum to mean |U|^2"""
    U = gpu_util.white_cpu((2, 1, 6, 10), seed=1).to(torch.complex128)
    eta = ref.orders(U, tuple(range(10)), tuple(range(6)))
    assert torch.allclose(eta.sum((-2, -1)), U.abs().pow(2).mean((-2, -1)), rtol=1e-13, atol=0)


def test_obliquity_against_rayleigh_sommerfeld():
    """the obliquity form is r exp(-i k r) times the Rayleigh-Sommerfeld sum at r (u, v, w), r = 1e3 m, for a 16 x 16
    aperture of 0.5 mm at lambda = 1 mm; rho is the largest pixel radius and the bound
    2 (k rho^2 / (2 r) + 3 rho / r + 1 / (k r)) the first neglected terms of the expansion, doubled for the next order"""
    n, pitch, lam, r = 16, 0.5e-3, 1e-3, 1e3
    k = 2 * math.pi / lam
    U = gpu_util.white_cpu((1, 1, n, n), seed=2).to(torch.complex128)
    dirs = torch.tensor([[0.0, 0.0], [0.3, -0.2], [-0.6, 0.5], [0.1, 0.7]], dtype=torch.float64)
    s = torch.tensor([1 / lam], dtype=torch.float64)
    Ex, Ey = ref.table(n, pitch, 0.0, dirs[:, 0], s), ref.table(n, pitch, 0.0, dirs[:, 1], s)
    far = ref.list_forward(Ey, U, Ex, pitch * pitch, ref.oblique(dirs[:, 0], dirs[:, 1], s))
    w = torch.sqrt(1 - (dirs ** 2).sum(-1))
    pts = r * torch.cat([dirs, w[:, None]], -1)
    rs = points_ref.rs_points(U, pts, torch.tensor([lam], dtype=torch.float64), (pitch, pitch)) * r * cmath_exp(-k * r)
    rho = math.hypot(pitch * (n - 1) / 2, pitch * (n - 1) / 2)
    bound = 2 * (k * rho * rho / (2 * r) + 3 * rho / r + 1 / (k * r))
    err = float((far - rs).abs().max() / far.abs().max())
    print(f"obliquity vs Rayleigh-Sommerfeld: err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
    assert err <= bound


def cmath_exp(phase):
    """exp(i phase) with the phase reduced in turns first: k r = 6e6 rad"""
    t = phase / (2 * math.pi)
    return complex(math.cos(2 * math.pi * (t - round(t))), math.sin(2 * math.pi * (t - round(t))))
