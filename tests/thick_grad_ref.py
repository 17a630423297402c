"""The backward of the thick-element DOE model (thz_thick_backward) restated on the CPU, by hand.

Built on tests/thick_ref.py.  One step is A = crop F^-1 diag(H_dz) F pad, so A^H is the same with conj(H_dz)
(tests/table_ref.asm_adjoint_from_table).  d_s = clamp(h - z_s, 0, dz) moves with h only in the slab the
height ends in (the pixel's active slab), where t_s' = kappa_c t_s with
  kappa_c = -(k_c/2) tand sqrt(eps) + sign i k_c (sqrt(eps) - 1).
With V_s = U_s t_s and gU_S = G:
  gV_s = A^H gU_{s+1},  gU_s = conj(t_s) gV_s,  g_h(p) = sum_bc Re(conj(kappa_c V_{s(p)}(p)) gV_{s(p)}(p)).
The forward keeps one stash, V_s(p) where s is the active slab of p, as the saving kernels do; no torch
autograd is used anywhere in this file.

``dtype=torch.complex128``: everything in fp64, the active slab from the exact faces (0 < h - s dz < dz).
``dtype=torch.complex64``: the kernels' fp32 arithmetic -- thick_ref's fp32 screens, kappa in
doe_transmission's operation order, the active slab from the fp32 faces with the kernels' tie rule (of two
neighbouring slabs that both pass, the upper one), fp32 partials -- and, like the kernels' closing reduction,
fp64 sums over b, c and the upsample footprint.  It is the floor the GPU bounds are multiples of.

Plain helper module: no test, no fixture, torch and numpy only.
"""
import numpy as np
import torch

from tests import table_ref as tr
from tests import thick_ref as th

C128 = torch.complex128


def interior_heights(hs, ws, thickness, slices, seed=0):
    """thick_ref.boundary_heights with every entry that sits exactly on a face, on 0 or on T moved half a
    slab inward; the entries below 0 and above T are kept (their gradient is exactly 0)."""
    h = th.boundary_heights(hs, ws, thickness, slices, seed)
    dz = th.step_size(thickness, slices)
    flat = h.reshape(-1)
    flat[0] += np.float32(0.5 * dz)                   # 0
    flat[2] -= np.float32(0.5 * dz)                   # T
    flat[4] += np.float32(0.5 * dz)                   # z_0 = 0
    flat[5:4 + slices] -= np.float32(0.5 * dz)        # z_1 .. z_{S-1}
    return h


def active_slab(hf, thickness, slices, rdt):
    """[S, H, W] bool: slab s is the active slab of the pixel.  At most one per pixel."""
    dz = th.step_size(thickness, slices)
    if rdt == torch.float64:
        x = [hf.to(rdt) - s * dz for s in range(slices)]
        return torch.stack([(v > 0) & (v < dz) for v in x])
    dzf = float(np.float32(dz))
    inside = []
    for s in range(slices):
        v = hf.float() - float(np.float32(s * dz))
        inside.append((v > 0) & (v < dzf))
    inside.append(torch.zeros_like(inside[0]))
    return torch.stack([inside[s] & ~inside[s + 1] for s in range(slices)])


def kappa(wavelengths, eps, tand, sign, dtype):
    """kappa_c [C, 1, 1] complex"""
    rdt = torch.float64 if dtype == C128 else torch.float32
    lam = torch.tensor([float(np.float32(w)) for w in wavelengths], dtype=rdt)[:, None, None]
    se = torch.sqrt(torch.tensor(float(np.float32(eps)), dtype=rdt))
    td = torch.tensor(float(np.float32(tand)), dtype=rdt)
    if rdt == torch.float64:
        k = 2 * torch.pi / lam
        return torch.complex(-0.5 * k * td * se, sign * k * (se - 1))
    k = torch.tensor(6.283185307179586, dtype=rdt) / lam   # doe_transmission's gamma
    return torch.complex(((-0.5 * k) * td) * se, -sign * (-k * (se - 1.0)))


def forward_saved(x, height, Hc, wavelengths, eps, tand, thickness, slices, ph, pw, sign=-1.0, dtype=C128):
    """-> (U_S, stash [B,C,H,W], active [S,H,W]); stash holds V_s where slab s is active, 0 elsewhere.
    ``height`` may be float64 (the finite-difference test perturbs it below fp32 resolution)."""
    rdt = torch.float64 if dtype == C128 else torch.float32
    H, W = x.shape[-2:]
    hf = th.upsample(height, H, W)
    d = th.slab_thicknesses(hf, thickness, slices, rdt)
    act = active_slab(hf, thickness, slices, rdt)
    u = x.to(dtype)
    stash = torch.zeros_like(u)
    for s in range(slices):
        v = u * th.screen(d[s], wavelengths, eps, tand, sign, s == 0, dtype)[None]
        stash = torch.where(act[s], v, stash)
        u = tr.asm_from_table(v, Hc, ph, pw, True, dtype)
    return u, stash, act


def backward(G, height, Hc, stash, act, wavelengths, eps, tand, thickness, slices, ph, pw, sign=-1.0, dtype=C128):
    """-> (grad_field [B,C,H,W], grad_height [hs,ws] float64) of Re<out, G>."""
    rdt = torch.float64 if dtype == C128 else torch.float32
    H, W = G.shape[-2:]
    hs, ws = height.shape
    hf = th.upsample(height, H, W)
    d = th.slab_thicknesses(hf, thickness, slices, rdt)
    kap = kappa(wavelengths, eps, tand, sign, dtype)
    g = G.to(dtype)
    part = torch.zeros(g.shape, dtype=rdt)
    for s in reversed(range(slices)):
        gv = tr.asm_adjoint_from_table(g[None], [Hc], ph, pw, True, dtype)
        part = torch.where(act[s], ((kap * stash).conj() * gv).real, part)
        g = th.screen(d[s], wavelengths, eps, tand, sign, s == 0, dtype)[None].conj() * gv
    per_pixel = part.double().sum((0, 1))   # fp64 sums, as the closing reduction
    gh = torch.zeros(hs, W, dtype=torch.float64).index_add_(0, th.nearest_index(hs, H), per_pixel)
    gh = torch.zeros(hs, ws, dtype=torch.float64).index_add_(1, th.nearest_index(ws, W), gh)
    return g, gh


def gradients(x, height, Hc, G, wavelengths, eps, tand, thickness, slices, ph, pw, sign=-1.0, dtype=C128):
    """(out, grad_field, grad_height) of L = Re<out, G> = sum Re(out conj(G))."""
    out, stash, act = forward_saved(x, height, Hc, wavelengths, eps, tand, thickness, slices, ph, pw, sign, dtype)
    gx, gh = backward(G, height, Hc, stash, act, wavelengths, eps, tand, thickness, slices, ph, pw, sign, dtype)
    return out, gx, gh


def autograd_gradients(x, height, Hc, G, wavelengths, eps, tand, thickness, slices, ph, pw, sign=-1.0):
    """The same three by torch autograd of thick_ref.thick_from_table in fp64."""
    x64 = x.to(C128).clone().requires_grad_(True)
    h = height.double().clone().requires_grad_(True)   # a float64 leaf: its grad is not rounded to fp32
    out = th.thick_from_table(x64, h, Hc, wavelengths, eps, tand, thickness, slices, ph, pw, sign=sign)
    (out * G.to(C128).conj()).real.sum().backward()
    return out.detach(), x64.grad, h.grad


def rel_l2(got, ref):
    return float((got.to(ref.dtype) - ref).norm() / ref.norm())
