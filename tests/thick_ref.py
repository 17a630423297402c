"""The thick-element DOE model (optics.thick_doe, thz_thick_forward) restated on the CPU.

dz = T / S, z_s = s dz, d_s = clamp(h_full - z_s, 0, dz) (d_0 also carries the base plate b),
t_{c,s} = exp(-k_c/2 d_s tand sqrt(eps)) exp(sign i k_c d_s (sqrt(eps) - 1)), U_{s+1} = A_dz(U_s t_s).

The step A_dz is tests/table_ref.asm_from_table around a transfer function that is handed in (the
table ASM_prop.create_kernel exports for z = dz, or the oracle's fp64 one), so the rounding of the
table's phase argument cancels against a HIP result, as in tests/test_table_parity_gpu.py.

``dtype=torch.complex128`` (the default) is the fp64 restatement: the fp32 inputs (map, thickness,
wavelengths, eps, tand) promoted, everything else in fp64; differentiable in ``height`` and ``x``.
``dtype=torch.complex64`` runs the same algebra in fp32 in the kernels' op order (doe_transmission of
csrc/thz_dev.hpp: z_s and dz rounded to fp32, slabs above the first formed as (d_s - b) + b, torch's
fp32 exp / sin / cos and CPU FFT): the yardstick the GPU tolerances are multiples of.

Plain helper module: no test, no fixture, torch and numpy only.
"""
import numpy as np
import torch

from tests import table_ref as tr

C128 = torch.complex128
BASE32 = float(np.float32(2e-3))  # DOE_BASE_PLANE as the kernels hold it


def nearest_index(n_in, n_out):
    """doe_nearest_src: torch's mode='nearest' source index with an fp32 scale."""
    if n_in == n_out:
        return torch.arange(n_out)
    scale = np.float32(n_in) / np.float32(n_out)
    idx = np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64)
    return torch.from_numpy(np.minimum(idx, n_in - 1))


def upsample(h, H, W):
    return h.index_select(0, nearest_index(h.shape[0], H)).index_select(1, nearest_index(h.shape[1], W))


def step_size(thickness, slices):
    """dz in double from the fp32 thickness, as the library forms it"""
    return float(np.float32(thickness)) / slices


def slab_thicknesses(h, thickness, slices, dtype=torch.float64):
    """[S, *h.shape]: d_s = clamp(h - z_s, 0, dz) without the base plate.  fp64: exact z_s and dz;
    fp32: both rounded to fp32 first, as the kernels receive them."""
    dz = step_size(thickness, slices)
    h = h.to(dtype)
    out = []
    for s in range(slices):
        zs, dzs = s * dz, dz
        if dtype == torch.float32:
            zs, dzs = float(np.float32(zs)), float(np.float32(dzs))
        out.append((h - zs).clamp(0.0, dzs))
    return torch.stack(out)


def screen(d, wavelengths, eps, tand, sign, first, dtype=C128, base=BASE32):
    """t_{c,s} [C, H, W] of one slab thickness d [H, W] (``first``: the slab on the base plate)."""
    rdt = torch.float64 if dtype == C128 else torch.float32
    lam = torch.tensor([float(np.float32(w)) for w in wavelengths], dtype=rdt)[:, None, None]
    b = torch.tensor(base, dtype=rdt)
    se = torch.sqrt(torch.tensor(float(np.float32(eps)), dtype=rdt))
    td = torch.tensor(float(np.float32(tand)), dtype=rdt)
    if rdt == torch.float64:
        k = 2 * torch.pi / lam
        hb = (d + b if first else d)[None]
        loss = torch.exp(-0.5 * k * hb * td * se)
        ph = sign * k * hb * (se - 1)
    else:  # doe_transmission's op order on hv = d (first slab) or d - b
        k = torch.tensor(6.283185307179586, dtype=rdt) / lam
        hb = ((d if first else d - b) + b)[None]
        loss = torch.exp(((-0.5 * k) * hb * td) * se)
        ph = -sign * ((-k * hb) * (se - 1.0))
    return torch.complex(loss * torch.cos(ph), loss * torch.sin(ph))


def thick_from_table(x, height, Hc, wavelengths, eps, tand, thickness, slices, ph, pw, sign=-1.0, dtype=C128,
                     base=BASE32):
    """x [B,C,H,W], height [hs,ws] float32, Hc [1,C,Ph,Pw] (H of one step dz, centred grid) -> U_S [B,C,H,W]."""
    rdt = torch.float64 if dtype == C128 else torch.float32
    H, W = x.shape[-2:]
    d = slab_thicknesses(upsample(height, H, W), thickness, slices, rdt)
    u = x.to(dtype)
    for s in range(slices):
        t = screen(d[s], wavelengths, eps, tand, sign, s == 0, dtype, base)
        u = tr.asm_from_table(u * t[None], Hc, ph, pw, True, dtype)
    return u


def floor_of(lo, ref, slices):
    """errors() of the complex64 run against the complex128 run, checked to be what a bound may rest
    on: no better than one fp32 rounding, and per slab no worse than an fp32 FFT pipeline (2e-6 / 2e-5,
    tests/table_ref.floor_of) plus a screen whose phase argument k (d + b)(sqrt(eps) - 1) of up to 20 rad
    rounds by about 1e-6 rad -- twice table_ref's caps per slab."""
    rel, mx = tr.errors(lo, ref)
    assert 2.0 ** -24 <= rel <= 4e-6 * slices and rel <= mx <= 4e-5 * slices, \
        f"floor32 {rel:.3e} {mx:.3e} is not an fp32 pipeline's error over {slices} slabs"
    return rel, mx


def boundary_heights(hs, ws, thickness, slices, seed=0):
    """A map [hs, ws] of random heights in [-0.1 T, 1.1 T] whose first entries are the boundary values:
    0, below 0, exactly every z_s (as fp32), T, above T."""
    g = torch.Generator().manual_seed(seed)
    h = ((torch.rand(hs, ws, generator=g) * 1.2 - 0.1) * thickness).float()
    dz = step_size(thickness, slices)
    vals = [0.0, -0.25 * thickness, float(np.float32(thickness)), 1.5 * thickness] + [s * dz for s in range(slices)]
    flat = h.reshape(-1)
    assert len(vals) <= flat.numel()
    flat[:len(vals)] = torch.tensor(vals, dtype=torch.float32)
    return h
