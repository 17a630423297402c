"""The RSC / VRS z-x slice cases: geometries, sweep, seeded inputs, fields and the fp64 oracle's planes, shared by
tests/test_rsc_zx_gpu.py, tests/test_rsc_zx_grad_gpu.py, tests/test_table_parity_gpu.py and tests/test_table_ref_cpu.py.

Plain helper module: no test, no fixture.  Inputs are seeded complex white noise; the oracle sees the fp32-rounded
wavelengths, spacings and distances the kernels are given.
"""
import functools

import torch

from oracle import thz_oracle as orc
from tests.gpu_util import dev, f32

# (H, W, C, B, (dx, dy)): H != W and dx != dy, C and B above 1, odd sizes (Pw = 93, Ph = 65), lines
# that are no multiple of 64 -- all on the runtime FFT plan (Pw = 200, 93, 140, 48)
GEOMETRIES = [
    (72, 100, 2, 1, (0.25e-3, 0.3e-3)),
    (33, 47, 1, 2, (0.25e-3, 0.25e-3)),
    (130, 70, 3, 1, (0.25e-3, 0.25e-3)),
    (20, 24, 1, 1, (0.5e-3, 0.5e-3)),
]
# the compile-time plans Pw = 1024, 2048, 4096 and 8192 (last-stage radices 4, 8, 16, 2; no transform
# runs along H: H stays tiny), and Pw = 16384, whose accumulate kernel runs the runtime plan next to
# compile-time row and line kernels
PLANS = [
    (24, 512, 1, 1, (0.25e-3, 0.25e-3)),
    (16, 1024, 1, 1, (0.25e-3, 0.25e-3)),
    (4, 8192, 1, 1, (0.25e-3, 0.25e-3)),
    (4, 2048, 1, 1, (0.25e-3, 0.25e-3)),
    (4, 4096, 1, 1, (0.25e-3, 0.25e-3)),
]
# more than one output plane per call (through rsc_slice_apply): a runtime-plan width inside
# [1024, 8192] (Pw = 1200: one plane per accumulate workgroup), and the compile-time tiles of two
# (B = 2; B = 4: two tiles of two) and three planes (B = 5: tiles of three and two, one slot idle)
BATCHES = [
    (8, 600, 1, 2, (0.25e-3, 0.25e-3)),
    (8, 512, 1, 2, (0.25e-3, 0.25e-3)),
    (6, 512, 1, 4, (0.25e-3, 0.25e-3)),
    (6, 512, 1, 5, (0.25e-3, 0.25e-3)),
]
VRS = (40, 48, 2, 2, (0.25e-3, 0.3e-3))      # Ex, Ey planes in, three planes out; Pw = 96
VRS_PLAN = (12, 512, 1, 2, (0.25e-3, 0.25e-3))   # Pw = 1024: three planes per accumulate workgroup
VRS_1200 = (8, 600, 2, 2, (0.25e-3, 0.25e-3))    # Pw = 1200: the runtime plan inside [1024, 8192]
VRS_4096 = (4, 2048, 1, 2, (0.25e-3, 0.25e-3))   # Pw = 4096: the radix-16 last stage, three planes
ZS = (0.030, 0.041, 0.055, 0.0725, 0.090)   # 30 ... 90 mm, not uniformly spaced


def synthetic_lam(C):
    return [1e-3 * (1 + 0.1 * c) for c in range(C)]


def rows(n):
    return (0, n // 2, n - 1)


def case_id(g):
    return f"{g[0]}x{g[1]}" + (f"xB{g[3]}" if g[3] > 2 else "")


@functools.lru_cache(maxsize=None)
def white_input(geo, dtype=torch.complex64):
    H, W, C, B = geo[:4]
    g = torch.Generator().manual_seed(1000 * H + W)
    return torch.randn(B, C, H, W, dtype=torch.complex128, generator=g).to(dtype)


def field(geo, dtype=torch.complex64, grad=False, data=None):
    from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
    C, spacing = geo[2], geo[4]
    data = (white_input(geo, dtype) if data is None else data).to(dev())
    if grad:
        data.requires_grad_(True)
    wl = synthetic_lam(C)
    if dtype == torch.complex128:
        wl = torch.tensor(wl, dtype=torch.float64)
    elif C == 1:
        wl = wl[0]
    return ElectricField(data, wavelengths=wl, spacing=list(spacing), device=dev())


def prop(vectorial=False):
    from quantizationawarethzdoe_amd.Props.RSC_Prop import RSC_prop, VRS_prop
    return (VRS_prop if vectorial else RSC_prop)(z_distance=0.05, device=dev())


@functools.lru_cache(maxsize=None)
def oracle_planes(geo, zs, vectorial=False, exact=False):
    """fp64 oracle planes [Z, Bo, C, Ho, Wo] (computed once per geometry and sweep, never modified) at
    the values the kernels are given: fp32 roundings, or with ``exact`` (the complex128 test) the
    doubles themselves except the spacing, which ElectricField stores as float32.  VRS: Ez = Ex x / r +
    Ey y / r on the unpadded grid, then the scalar convolution per component
    (test_vrs_matches_oracle_componentwise)."""
    H, W, C, B, spacing = geo
    dx, dy = f32(spacing[0]), f32(spacing[1])
    r = (lambda v: v) if exact else f32
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        x = white_input(geo, torch.complex128 if exact else torch.complex64).to(torch.complex128)
        lam = torch.tensor([r(v) for v in synthetic_lam(C)])
        planes = []
        for z in zs:
            z = r(z)
            v = x
            if vectorial:
                xs = torch.linspace(-H * dx / 2, H * dx / 2, H)
                ys = torch.linspace(-W * dx / 2, W * dx / 2, W)
                X, Y = torch.meshgrid(xs, ys, indexing="ij")
                rr = torch.sqrt(X ** 2 + Y ** 2 + z ** 2)
                v = torch.cat([x[0:1], x[1:2], x[0:1] * X / rr + x[1:2] * Y / rr], 0)
            planes.append(torch.cat([orc.rsc_forward(v[b:b + 1], lam, [dx, dy], z) for b in range(v.shape[0])], 0))
        return torch.stack(planes)
    finally:
        torch.set_default_dtype(old)
