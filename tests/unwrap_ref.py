"""A torch restatement of the unwrapping model of include/thzdoe.h (thz_unwrap_*) on the CPU, callable in float64 and
float32.  Its cosine transforms go by the FFT of the mirrored 2N extension, so it shares nothing with the kernels'
two-lines-per-transform packing.  Plain helper module: no test, no fixture.
"""
import math

import torch

TWO_PI = 2 * math.pi


def dct2(x, dim):
    """X[k] = sum_n x[n] cos(pi (2n + 1) k / 2N) along ``dim``"""
    x = x.movedim(dim, -1)
    N = x.shape[-1]
    Y = torch.fft.fft(torch.cat([x, x.flip(-1)], -1), dim=-1)[..., :N]
    k = torch.arange(N, dtype=torch.float64)
    ph = torch.polar(torch.ones(N, dtype=torch.float64), -math.pi * k / (2 * N)).to(Y.dtype)
    return ((Y * ph).real / 2).movedim(-1, dim)


def idct2(X, dim):
    """the inverse of dct2: x[n] = (X[0] + 2 sum_{k >= 1} X[k] cos(pi (2n + 1) k / 2N)) / N"""
    X = X.movedim(dim, -1)
    N = X.shape[-1]
    k = torch.arange(N, dtype=torch.float64)
    ph = torch.polar(torch.full((N,), 2.0, dtype=torch.float64), math.pi * k / (2 * N))
    Y = X.to(torch.complex128 if X.dtype == torch.float64 else torch.complex64) * ph.to(
        torch.complex128 if X.dtype == torch.float64 else torch.complex64)
    Y = torch.cat([Y, torch.zeros_like(Y[..., :1])], -1)
    return torch.fft.irfft(Y, n=2 * N, dim=-1)[..., :N].movedim(-1, dim)


def _side(n):
    p = 64
    while p < n:
        p *= 2
    return p


def wrapped_diffs(x, dtype):
    """(Dx [..., H, W - 1], Dy [..., H - 1, W]) of a complex field or a real wrapped phase, formed in ``dtype``"""
    if x.is_complex():
        U = x.to(torch.complex128 if dtype == torch.float64 else torch.complex64)
        return (torch.angle(U[..., :, 1:] * U[..., :, :-1].conj()), torch.angle(U[..., 1:, :] * U[..., :-1, :].conj()))
    p = x.to(dtype)
    dx, dy = p[..., :, 1:] - p[..., :, :-1], p[..., 1:, :] - p[..., :-1, :]
    return dx - TWO_PI * torch.round(dx / TWO_PI), dy - TWO_PI * torch.round(dy / TWO_PI)


def psi_of(x, dtype):
    return torch.angle(x.to(torch.complex128 if dtype == torch.float64 else torch.complex64)) if x.is_complex() \
        else x.to(dtype)


def unwrap(x, weights=None, iters=0, tol=1e-6, congruent=False, anchor=None, dtype=torch.float64):
    """(phi [..., H, W], hist [iters, planes] or None): the model, planes embedded in power-of-two sides from 64 with
    weight 0 on the padding.  ``weights``: None, "amplitude", "intensity" or a tensor; ``anchor``: None or (row, col)."""
    H, W = x.shape[-2:]
    PH, PW = _side(H), _side(W)
    lead = tuple(x.shape[:-2])
    if weights is None:
        w = torch.ones(lead + (H, W), dtype=dtype)
    elif isinstance(weights, str):
        a = x.to(torch.complex128).abs() ** (2 if weights == "intensity" else 1)
        w = (a / a.amax((-2, -1), keepdim=True)).to(dtype)
    else:
        w = weights.to(dtype).expand(lead + (H, W))
    dx, dy = wrapped_diffs(x, dtype)
    wp = torch.zeros(lead + (PH, PW), dtype=dtype)
    wp[..., :H, :W] = w
    wx, wy = torch.minimum(wp[..., :, :-1], wp[..., :, 1:]), torch.minimum(wp[..., :-1, :], wp[..., 1:, :])
    gx, gy = torch.zeros(lead + (PH, PW), dtype=dtype), torch.zeros(lead + (PH, PW), dtype=dtype)
    gx[..., :H, :W - 1] = torch.where(wx[..., :H, :W - 1] > 0, wx[..., :H, :W - 1] * dx, torch.zeros_like(dx))
    gy[..., :H - 1, :W] = torch.where(wy[..., :H - 1, :W] > 0, wy[..., :H - 1, :W] * dy, torch.zeros_like(dy))
    rho = gx.clone()
    rho[..., :, 1:] -= gx[..., :, :-1]
    rho += gy
    rho[..., 1:, :] -= gy[..., :-1, :]

    def s(n):
        return (4 * torch.sin(math.pi * torch.arange(n, dtype=torch.float64) / (2 * n)) ** 2).to(dtype)
    lam = -(s(PH)[:, None] + s(PW)[None, :])
    lam[0, 0] = 1

    def pinv(r):
        c = dct2(dct2(r, -1), -2) / lam
        c[..., 0, 0] = 0
        return idct2(idct2(c, -2), -1).to(dtype)

    def Q(p):
        ex, ey = wx * (p[..., :, 1:] - p[..., :, :-1]), wy * (p[..., 1:, :] - p[..., :-1, :])
        q = torch.zeros_like(p)
        q[..., :, :-1] += ex
        q[..., :, 1:] -= ex
        q[..., :-1, :] += ey
        q[..., 1:, :] -= ey
        return q

    def dot(a, b):  # -(a . b) per plane, summed in float64 as the kernels' partials are
        return -(a.double() * b.double()).sum((-2, -1), keepdim=True)

    hist = None
    if iters == 0:
        phi = pinv(rho)
    else:
        phi, r, p = torch.zeros_like(rho), rho.clone(), torch.zeros_like(rho)
        rz_old = rz0 = None
        hist = []
        for k in range(iters):
            z = pinv(r)
            rz = dot(r, z)
            rz0 = rz if k == 0 else rz0
            frozen = ~(rz > tol * tol * rz0) | ~torch.isfinite(rz)
            beta = torch.zeros_like(rz) if k == 0 else torch.where(frozen | ~(rz_old > 0), torch.zeros_like(rz),
                                                                   rz / rz_old)
            p = z + beta.to(dtype) * p
            qp = Q(p)
            pqp = dot(p, qp)
            alpha = torch.where(frozen | ~(pqp > 0) | ~torch.isfinite(pqp), torch.zeros_like(rz), rz / pqp).to(dtype)
            phi, r, rz_old = phi + alpha * p, r - alpha * qp, rz
            hist.append(torch.where(rz0 > 0, (rz.clamp_min(0) / rz0).sqrt(), torch.zeros_like(rz)).reshape(-1))
        hist = torch.stack(hist)
    phi = phi[..., :H, :W]
    psi = psi_of(x, dtype)
    if anchor is not None:
        ar, ac = anchor
        phi = phi + (psi[..., ar:ar + 1, ac:ac + 1] - phi[..., ar:ar + 1, ac:ac + 1])
    if congruent:
        phi = psi + TWO_PI * torch.round((phi - psi) / TWO_PI)
    return phi, hist


# ---- the inputs of the tests ---------------------------------------------------------------------------------
def smooth_field(H, W, seed=0):
    """(complex64 field, its true phase float64): s = x^2 + 1.5 y^2 + 0.4 x - 0.3 y + 0.5 x y on [-1, 1]^2 scaled to a
    largest neighbour difference of 2.5 rad, under a random amplitude in [0.2, 1.2]"""
    y, x = torch.meshgrid(torch.linspace(-1, 1, H, dtype=torch.float64), torch.linspace(-1, 1, W, dtype=torch.float64),
                          indexing="ij")
    s = x * x + 1.5 * y * y + 0.4 * x - 0.3 * y + 0.5 * x * y
    s = s * (2.5 / max(float((s[:, 1:] - s[:, :-1]).abs().max()), float((s[1:] - s[:-1]).abs().max())))
    amp = 0.2 + torch.rand(H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))
    return torch.polar(amp, s).to(torch.complex64), s


def speckle(shape, seed=1, sigma=0.08):
    """complex normal noise low-passed by a Gaussian of ``sigma`` cycles per pixel: it holds real residues"""
    n = torch.randn(*shape, dtype=torch.complex128, generator=torch.Generator().manual_seed(seed))
    fy, fx = torch.fft.fftfreq(shape[-2], dtype=torch.float64), torch.fft.fftfreq(shape[-1], dtype=torch.float64)
    g = torch.exp(-(fy[:, None] ** 2 + fx[None, :] ** 2) / (2 * sigma * sigma))
    return torch.fft.ifft2(torch.fft.fft2(n) * g).to(torch.complex64)


def holed_field(H=80, W=96, seed=2):
    """(complex64 field, true phase, weights): 0.012 x^2 + 0.02 y^2 + 0.3 x - 0.2 y in pixels from the centre, a disk
    of radius 12 at (+10, -7) from the centre filled with uniform random phase and given weight 0"""
    i, j = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    y, x = i - H // 2, j - W // 2
    s = 0.012 * x * x + 0.02 * y * y + 0.3 * x - 0.2 * y
    hole = (y - 10) ** 2 + (x + 7) ** 2 <= 144
    junk = TWO_PI * torch.rand(H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))
    return torch.polar(torch.ones_like(s), torch.where(hole, junk, s)).to(torch.complex64), s, (~hole).to(torch.float32)
