"""CZT parity, the CPU side: a plain torch reference of CZT_prop, independent of the kernels.

The chirp-z propagator forms its chirps in-kernel and exports no table, so unlike tests/table_ref.py
nothing is handed in: czt_forward restates oracle/thz_oracle.py (_rs_kernel, _bluestein, czt_forward:
the reference's [m : m + M] slice, its post-chirp h[m - 1 : m - 1 + M], M_shift, and Dm = lambda z /
dx on BOTH axes) with two switches.

``grids``: the coordinates x_in, y_in, x_out, y_out.  "fp64": float64 linspace, the oracle run with a
float64 default dtype.  "fp32": float32 ``torch.linspace`` cast to double, formed element by element
(lin32) -- the grid values the reference's fp32 run on a GPU and the kernels' ``lin()``
(csrc/thz_dev.hpp) work on; everything downstream of those values stays fp64.  An ulp of a coordinate
moves the RS phase k rho^2 / (r + |z|) by 2^-23 of itself (1e-4 rad at 10^3 rad), so a tight
comparison has to start from the same grid values.

``dtype``: complex128 is the truth.  complex64 is floor32: the RS factors on both meshes, the scalar
z odx ody lambda, the pre chirp A^-j h, the filter spectrum FFT(1 / h) and the post chirp h M_shift
are computed in fp64 exactly as for the truth and rounded once to complex64 (float32); the data path
(products, the two np2 transforms per pass on torch's CPU FFT, the slice) runs in complex64.  It is
the error of a correctly rounded fp32 pipeline around exact tables: what an fp32 kernel can reach.

Differentiable in both dtypes: the adjoint reference is ``torch.autograd.grad`` through czt_forward
(czt_grad).  All spacings, z and wavelengths are rounded to float32 on entry (idempotent on values a
launch already received) and promoted; ``as_given`` keeps odx, ody and z as the doubles the complex128
entry receives.

Plain helper module: no test, no fixture, torch only.  tests/test_czt_ref_cpu.py pins it against the
oracle.
"""
import math

import torch

C128 = torch.complex128
C64 = torch.complex64
U32 = 2.0 ** -24   # one fp32 rounding, relative


def f32(v):
    """v rounded to float32, as a Python float"""
    return float(torch.tensor(float(v), dtype=torch.float32))


def lin32(start, end, n):
    """float32 torch.linspace(start, end, n) element by element: start + step i below n // 2, end -
    step (n - 1 - i) from there on, step = (end - start) / (n - 1), each operation rounded to float32.
    That is ATen's definition, what torch's GPU kernel evaluates and what the kernels' ``lin()`` restates.
    torch's CPU kernel evaluates it in 8-wide chunks (chunk base + step lane: one rounding more) and
    lands an ulp away on some elements, so the float32 grid is formed here, not by the CPU linspace."""
    start, end = torch.tensor(start, dtype=torch.float32), torch.tensor(end, dtype=torch.float32)
    if n == 1:
        return start.reshape(1)
    step = (end - start) / torch.tensor(n - 1, dtype=torch.float32)
    i = torch.arange(n)
    lo = i < n // 2
    return torch.where(lo, start, end) + step * torch.where(lo, i, i - (n - 1)).to(torch.float32)


def _lin(n, d, grids):
    """linspace(-n d / 2, n d / 2, n) as float64 values: formed in float32 (``grids="fp32"``) or float64"""
    e = n * d / 2
    if grids == "fp32":
        return lin32(-e, e, n).double()
    if grids == "fp64":
        return torch.linspace(-e, e, n, dtype=torch.float64)
    raise ValueError(f"grids={grids!r}")


def np2_of(mp):
    """the reference's 2 ** ceil(log2 mp) (Props/CZT_Prop.py:120-130)"""
    return int(2 ** int(math.ceil(math.log2(mp))))


def _rs(z, mx, my, lam):
    """exp(ikr) z / (2 pi r^2) (1 / r - ik), [1, C, *mesh], float64 (oracle._rs_kernel)"""
    k = 2 * torch.pi / lam[None, :, None, None]
    r = torch.sqrt(mx ** 2 + my ** 2 + z ** 2)
    return torch.exp(1j * k * r) * (1 / (2 * torch.pi) * z / r ** 2 * (1 / r - 1j * k))


def _tables(m, M, f1, f2, Dm):
    """(pre [1,C,m,1], ft [1,C,np2,1], post [1,C,1,M]) of one Bluestein pass, complex128, in the
    oracle's operations (_bluestein): pre = A^-j h[m-1+j], ft = FFT_np2(1 / h[:mp+1]), post =
    h[m-1:mp] M_shift."""
    D1 = f1 + (M * Dm + f2 - f1) / (2 * M)
    D2 = f2 + (M * Dm + f2 - f1) / (2 * M)
    mp = m + M - 1
    np2 = np2_of(mp)
    A = torch.exp(1j * 2 * torch.pi * D1 / Dm)
    Wc = torch.exp(-1j * 2 * torch.pi * (D1 - D2) / (M * Dm))
    jj = torch.arange(-m + 1, max(M - 1, m - 1) + 1, dtype=torch.float64)
    h = Wc ** (jj ** 2 / 2)
    ft = torch.fft.fft(1 / h[..., : mp + 1], n=np2, dim=-1)
    pre = A ** (-(torch.arange(0, m))) * h[..., torch.arange(m - 1, 2 * m - 1)]
    ell = torch.linspace(0, M - 1, M, dtype=torch.float64)[None, None, None, :]
    ell = ell / M * (D2 - D1) + D1
    shift = torch.exp(-1j * 2 * torch.pi * ell * (-m / 2 + 0.5) / Dm)
    post = h[..., m - 1:mp] * shift
    assert post.shape[-1] == M, "m + M - 1 is a power of two: the reference's slice keeps M - 1 rows"
    return pre.transpose(-2, -1), ft.transpose(-2, -1), post


def _ifft_rows(b):
    """ifft along dim -2 as conj(F conj(b)) / n: the unnormalised forward transform and an explicit
    product (tests/table_ref.py: the one form every CPU FFT back end gets right in complex64)"""
    return torch.fft.fft(b.conj(), dim=-2).conj() * (1.0 / b.shape[-2])


def _pass(x, tabs, M):
    """One Bluestein pass along dim -2 of x [B,C,m,n] -> [B,C,n,M] (the reference's transposed result)."""
    pre, ft, post = tabs
    m = x.shape[-2]
    b = torch.fft.fft(x * pre, n=ft.shape[-2], dim=-2)
    b = _ifft_rows(b * ft)
    return b[..., m:m + M, :].transpose(-2, -1) * post


class Case:
    """One CZT geometry: every factor and table czt_forward applies, complex128, formed once.

    H, W: the field; M: the square output (outH = outW = M); dx, dy / odx, ody: input / output
    pixels; z; lam: the wavelengths [C].  ``phase_in`` / ``phase_out`` [C]: the largest residual RS
    phase k rho^2 / (r + |z|) on the input / output mesh, the quantity the kernels round in fp32.
    ``as_given``: odx, ody and z stay the doubles they are, as the complex128 entry receives them."""

    def __init__(self, H, W, M, dx, dy, odx, ody, z, lam, grids="fp32", as_given=False):
        self.H, self.W, self.M = H, W, M
        dx, dy = f32(dx), f32(dy)   # ElectricField holds the spacing in float32
        if not as_given:            # the complex64 entry takes every scalar as a float
            odx, ody, z = f32(odx), f32(ody), f32(z)
        lam = torch.tensor([f32(v) for v in lam], dtype=torch.float64)
        zt = torch.tensor(z, dtype=torch.float64)
        xi, yi = _lin(H, dx, grids), _lin(W, dy, grids)
        xo, yo = _lin(M, odx, grids), _lin(M, ody, grids)
        imx, imy = torch.meshgrid(xi, yi, indexing="ij")
        omx, omy = torch.meshgrid(xo, yo, indexing="ij")
        Dm = lam[None, :, None, None] * zt / dx
        self.F = _rs(zt, imx, imy, lam)
        self.F0 = _rs(zt, omx, omy, lam)
        self.scale = (zt * odx * ody * lam)[None, :, None, None]
        # the reference's first pass runs along H with the y range, its second along W with the x range
        self.tab_h = _tables(H, M, yo[0] + Dm / 2, yo[-1] + Dm / 2, Dm)
        self.tab_w = _tables(W, M, xo[0] + Dm / 2, xo[-1] + Dm / 2, Dm)
        k = 2 * math.pi / lam

        def phase(a, b):
            rho2 = float(a.abs().max()) ** 2 + float(b.abs().max()) ** 2
            return k * rho2 / (math.sqrt(rho2 + z * z) + abs(z))

        self.phase_in, self.phase_out = phase(xi, yi), phase(xo, yo)

    def _as(self, dtype):
        """the factors in ``dtype``: complex64 rounds each of them once (the scalar to float32)"""
        if dtype == C128:
            return self.F, self.F0, self.scale, self.tab_h, self.tab_w
        assert dtype == C64
        return (self.F.to(C64), self.F0.to(C64), self.scale.to(torch.float32), tuple(t.to(C64) for t in self.tab_h),
                tuple(t.to(C64) for t in self.tab_w))

    def forward(self, x, dtype=C128):
        """x [B,C,H,W] -> [B,C,M,M] (the reference's [B,C,outW,outH]), computed in ``dtype``"""
        F, F0, scale, th, tw = self._as(dtype)
        assert tuple(x.shape[-2:]) == (self.H, self.W) and x.shape[1] == F.shape[1]
        U = x.to(dtype) * F
        U = _pass(U, th, self.M)
        U = _pass(U, tw, self.M)
        return F0 * U * scale

    def grad(self, x, g, dtype=C128):
        """(forward(x), A^H g): the adjoint by autograd through forward, as torch.autograd.grad of the
        propagator with grad_outputs = g gives it"""
        xg = x.detach().to(dtype).clone().requires_grad_(True)
        out = self.forward(xg, dtype)
        gin, = torch.autograd.grad(out, xg, grad_outputs=g.to(dtype))
        return out.detach(), gin


def czt_forward(x, lam, spacing, z, M, odx, ody, grids="fp32", dtype=C128):
    """CZT_prop.forward(field, M, M, odx, ody) on x [B,C,H,W] -> [B,C,M,M]"""
    H, W = x.shape[-2:]
    return Case(H, W, M, spacing[0], spacing[1], odx, ody, z, lam, grids).forward(x, dtype)


# ---------------------------------------------------------------------------------------------
# metrics, the fp32 floor and the bound
# ---------------------------------------------------------------------------------------------
def errors(got, ref):
    """(relative L2, max|err| / rms(ref)) of one plane, both taken in complex128 (tests/table_ref.py)"""
    got, ref = got.to(C128), ref.to(C128)
    err = (got - ref).abs()
    rms = float(ref.abs().pow(2).mean().sqrt())
    return float(err.pow(2).sum().sqrt() / ref.abs().pow(2).sum().sqrt()), float(err.max()) / rms


def floor_of(lo, ref):
    """errors() of the complex64 run ``lo`` against the complex128 run ``ref`` of one plane, checked to
    be what a bound may rest on: positive and below 1e-5 on both metrics.  A plane of one or two
    elements is a single draw of the rounding error and can land under one rounding by chance (3.7e-8
    at M = 1); no fp32 pipeline is expected to, so each figure is at least 2^-24."""
    rel, mx = errors(lo, ref)
    assert 0 < rel < 1e-5 and 0 < mx < 1e-5, f"floor32 {rel:.3e} {mx:.3e} is not an fp32 pipeline's error"
    return max(rel, U32), max(mx, U32)


def pass_form(m, M):
    """The form csrc/thz_czt.hip make_pass gives a forward pass of m inputs and M outputs: overlap-add
    when M fits half a 1024-point block and its nb + 1 transforms of 1024 points cost less than the np2
    pair, (nb + 1) 10240 < 2 np2 log2 np2"""
    nb = (m + 511) // 512
    n = np2_of(m + M - 1)
    return BLK if M <= 512 and (nb + 1) * 10240 < 2 * n * math.log2(n) else NP2


def plane_bounds_hold(case, got, x, forms):
    """Every (b, c) plane of ``got`` = A(x) within MARGIN x floor32 + PH on both metrics: (ok, worst
    err / bound, its description).  For drawn shapes, where a degenerate plane may have a zero floor."""
    ref, lo = case.forward(x), case.forward(x, C64)
    worst = (0.0, "")
    for b in range(ref.shape[0]):
        for c in range(ref.shape[1]):
            err = errors(got[b, c], ref[b, c])
            fl = errors(lo[b, c], ref[b, c])
            bnd = bound((max(fl[0], U32), max(fl[1], U32)), phase_term(case, c, *forms))
            r = max(err[0] / bnd[0], err[1] / bnd[1])
            if r > worst[0]:
                worst = (r, f"b{b} c{c} err {err[0]:.3e} {err[1]:.3e} bound {bnd[0]:.3e} {bnd[1]:.3e}")
    return worst[0] <= 1, worst[0], worst[1]


MARGIN = 4.0   # tests/test_table_parity_gpu.py: a different but equally valid fp32 FFT


def bound(floor, ph):
    """MARGIN x floor32 + PH on both metrics"""
    return MARGIN * floor[0] + ph, MARGIN * floor[1] + ph


# ---------------------------------------------------------------------------------------------
# the case matrix of tests/test_czt_parity_gpu.py (pinned on the CPU by tests/test_czt_ref_cpu.py)
# ---------------------------------------------------------------------------------------------
C0 = 2.998e8
GHZ = (300, 340, 380)
# geometry -> (dx, dy, odx, ody, z).  "tight": the residual RS phase stays near one radian, so its fp32
# rounding is of the order of floor32 and the Bluestein machinery is judged at 1e-6.  "physical": the
# suite's usual pixels (dy != dx, ody != odx) at z = 0.2 m, phases of 10 ... 10^3 rad on both meshes.
GEOMETRIES = {"tight": (0.02e-3, 0.02e-3, 0.03e-3, 0.025e-3, 0.5),
              "physical": (0.5e-3, 0.6e-3, 0.35e-3, 0.3e-3, 0.2)}
BLK, NP2 = "overlap-add", "np2"
# (H, W, M, B, C, form of pass A (W axis), form of pass B (H axis)): the smallest shapes that reach
# each path of csrc/thz_czt.hip make_pass; no m + M - 1 is a power of two
ROWS = [
    (37, 53, 15, 2, 2, NP2, NP2),       # odd sizes, np2 128 / 64, outH < 16: one partial V block
    (37, 53, 1, 2, 2, NP2, NP2),        # M = 1
    (40, 36, 17, 2, 3, NP2, NP2),       # outH = 17: a second V block holding one column
    (200, 1100, 24, 2, 2, BLK, NP2),    # mixed forms, A overlap-add (nb 3, partial last block), B np2 256
    (1100, 200, 24, 2, 2, NP2, BLK),    # mixed forms, B overlap-add (nb 3), its rs_kernel_fast on F0
    (1030, 1030, 2, 2, 3, BLK, BLK),    # the smallest np2 = 2048 overlap-add, M = 2, B x C = 2 x 3
    (1536, 40, 512, 1, 1, NP2, BLK),    # nb 3 with a full last block (PARTIAL = false), M at the cap
    (1536, 40, 17, 2, 2, NP2, BLK),     # the cost switch: nb 3 wins against np2 2048 ...
    (1537, 40, 17, 2, 2, NP2, NP2),     # ... and nb 4 loses
    (1100, 40, 513, 1, 1, NP2, NP2),    # M > 512: np2 whatever the cost
    (2100, 37, 17, 2, 2, NP2, BLK),     # the second overlap-add size class (nb 5 against np2 4096), odd H
    (1301, 1100, 256, 1, 3, BLK, BLK),  # odd H (no mirrored row pairs), an odd number of row pairs
]


def row_id(row):
    return f"{row[0]}x{row[1]}_M{row[2]}_B{row[3]}C{row[4]}"


def white(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, dtype=C128, generator=g).to(C64)


def wavelengths(C):
    return [f32(C0 / (f * 1e9)) for f in GHZ[:C]]


def build(row, geo, grids="fp32", as_given=False):
    """(Case, x [B,C,H,W] complex64 white noise, g [B,C,M,M] complex64 white noise) of a matrix entry"""
    H, W, M, B, C = row[:5]
    dx, dy, odx, ody, z = GEOMETRIES[geo]
    case = Case(H, W, M, dx, dy, odx, ody, z, wavelengths(C), grids, as_given)
    return case, white((B, C, H, W), 1000 * H + W + M), white((B, C, M, M), 77 + H + M)


# fp32 roundings on the way to the argument of the sine and cosine, counted in csrc/thz_dev.hpp:
# rs_kernel: x x, y y, their sum, z z, rho2 + z z, sqrtf, r + |z|, the division, the product with k,
# the sum with kzmod (10 correctly rounded operations) and the two constants k and kzmod rounded from
# double: 12.  rs_kernel_fast: the same sums and products with r = r2 rsq(r2) and rho2 rcp(r + |z|)
# (12 operations: the hardware rsq at one ulp counts twice, the Newton-refined rcp as its two fused
# steps) and the two constants: 16.  Each moves the phase by at most 2^-24 of itself, so the argument
# is off by at most ROUNDINGS 2^-24 phase, and exp(i phase) by as much.  Left out: the absolute error of
# the sine and cosine themselves (sincos_rad 6e-8, sincos_hw 1.8e-7) and the amplitude's roundings --
# one complex64 rounding's worth per factor, which floor32 pays too; MARGIN has to absorb them.
ROUNDINGS = {NP2: 12, BLK: 16}


def phase_term(case, c, form_in, form_out):
    """PH of plane wavelength c: the kernels' fp32 rounding of the residual RS phase, the larger of the
    input mesh's (the function pass A's form evaluates) and the output mesh's (pass B's form)"""
    return U32 * max(ROUNDINGS[form_in] * float(case.phase_in[c]), ROUNDINGS[form_out] * float(case.phase_out[c]))
