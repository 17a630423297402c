"""Table parity, the CPU side: the propagators' algebra on a table that is handed in.

Every propagator can export the fp32 table it applies (ASM_prop.create_kernel: the transfer function;
RSC_prop.create_kernel: the spatial RS kernel).  The functions below run pad -> FFT -> multiply ->
IFFT -> crop around such a table in complex128 with torch's CPU FFT, in the op order of
oracle/thz_oracle.py (asm_forward, rsc_forward; the normalisations as explicit products, see fft2u).  Nothing here forms a table: every one enters as an
argument, already on the CPU, and is promoted.  Against the result, the rounding of the table's phase
argument -- the term that dominates every oracle parity bound of the suite -- cancels, and what is left
of a HIP result is the kernels' own arithmetic.

``dtype=torch.complex64`` runs the identical algebra in fp32 (floor32): the reference arithmetic the
tolerances of tests/test_table_parity_gpu.py are measured against.

Plain helper module: no test, no fixture, torch only.  tests/test_table_ref_cpu.py pins it against the
oracle on the oracle's own fp64 tables.
"""
import torch

C128 = torch.complex128


def _real(dtype):
    return torch.float64 if dtype == torch.complex128 else torch.float32


# The 2-D transforms, one axis at a time through the unnormalised forward 1-D transform, the inverse as
# conj(F conj(x)), every normalisation an explicit product: the same values in exact arithmetic.  Some
# multi-threaded CPU FFT back ends apply the normalisation of a complex64 2-D transform twice from
# 2048 x 2048 on; their batched unnormalised 1-D transforms are sound, and floor32 must be an fp32 FFT.
def fft2u(x):
    return torch.fft.fft(torch.fft.fft(x, dim=-1), dim=-2)


def ifft2u(x):
    """N x ifft2(x)"""
    return fft2u(x.conj()).conj()


def ft2(x):
    """centred ortho 2-D FFT (oracle.thz_oracle.ft2)"""
    s = 1.0 / (x.shape[-2] * x.shape[-1]) ** 0.5
    return torch.fft.fftshift(fft2u(torch.fft.fftshift(x, dim=(-2, -1))) * s, dim=(-2, -1))


def ift2(x):
    """centred ortho inverse 2-D FFT (oracle.thz_oracle.ift2)"""
    s = 1.0 / (x.shape[-2] * x.shape[-1]) ** 0.5
    return torch.fft.ifftshift(ifft2u(torch.fft.ifftshift(x, dim=(-2, -1))) * s, dim=(-2, -1))


def _crop_origin(P, N):
    """the oracle's centre-crop offset (asm_forward)"""
    return int(round((P - N) / 2.0))


# ---------------------------------------------------------------------------------------------
# ASM: pad, centred FFT, x Hc, inverse, centre crop
# ---------------------------------------------------------------------------------------------
def asm_planes_from_tables(x, Hcs, ph, pw, unpad=True, dtype=C128):
    """x [B,C,H,W], Hcs: Z tables [1,C,Ph,Pw] on the centred grid (Ph = H + 2 ph, Pw = W + 2 pw) ->
    [Z,B,C,H,W] (the padded planes with ``unpad=False``).  The spectrum of the padded field does not
    depend on the plane and is formed once (oracle.thz_oracle.asm_forward_planes)."""
    x = x.to(dtype)
    H, W = x.shape[-2:]
    Ph, Pw = H + 2 * ph, W + 2 * pw
    spec = ft2(torch.nn.functional.pad(x, (pw, pw, ph, ph)) if (ph or pw) else x)
    planes = []
    for Hc in Hcs:
        assert tuple(Hc.shape[-2:]) == (Ph, Pw), (tuple(Hc.shape), Ph, Pw)
        y = ift2(spec * Hc.to(dtype))
        if unpad and (ph or pw):
            top, left = _crop_origin(Ph, H), _crop_origin(Pw, W)
            y = y[..., top:top + H, left:left + W]
        planes.append(y)
    return torch.stack(planes)


def asm_from_table(x, Hc, ph, pw, unpad=True, dtype=C128):
    """One plane: x [B,C,H,W], Hc [1,C,Ph,Pw] -> [B,C,H,W], or the padded plane with ``unpad=False``:
    pad, centred FFT, x Hc, inverse, centre crop."""
    return asm_planes_from_tables(x, [Hc], ph, pw, unpad, dtype)[0]


def asm_adjoint_from_table(g, Hcs, ph, pw, unpad=True, dtype=C128):
    """g [Z,B,C,Ho,Wo], Hcs: the Z tables [1,C,Ph,Pw] -> [B,C,H,W]: the sum over the planes of
    crop^T -> FFT -> conj(H_z) -> IFFT -> pad^T, the adjoint of asm_from_table per plane (the ortho
    centred transforms are each other's adjoints).  The planes are summed in the spectrum, before the
    one inverse transform: the same sum by linearity."""
    g = g.to(dtype)
    Z, B, C, Ho, Wo = g.shape
    Ph, Pw = Hcs[0].shape[-2:]
    H, W = Ph - 2 * ph, Pw - 2 * pw
    assert len(Hcs) == Z
    spec = torch.zeros((B, C, Ph, Pw), dtype=dtype)
    for k in range(Z):
        gp = g[k]
        if unpad and (ph or pw):
            assert (Ho, Wo) == (H, W)
            top, left = _crop_origin(Ph, H), _crop_origin(Pw, W)
            gp = torch.nn.functional.pad(gp, (left, Pw - W - left, top, Ph - H - top))
        assert tuple(gp.shape[-2:]) == (Ph, Pw)
        spec = spec + ft2(gp) * Hcs[k].to(dtype).conj()
    return ift2(spec)[..., ph:ph + H, pw:pw + W]


# ---------------------------------------------------------------------------------------------
# RSC / VRS: zero-embed, ifft2(fft2(U) fft2(K) dx dy), the far window
# ---------------------------------------------------------------------------------------------
def rsc_from_table(x, K, dx, dy, dtype=C128):
    """x [B,C,H,W], K [1,C,Ph,Pw] (the spatial RS kernel, Ph = H + 2 (H // 2)) -> [B,C,Ph-H,Pw-W]."""
    x, K = x.to(dtype), K.to(dtype)
    B, C, H, W = x.shape
    Ph, Pw = K.shape[-2:]
    assert (Ph, Pw) == (H + 2 * (H // 2), W + 2 * (W // 2))
    U = torch.zeros((B, C, Ph, Pw), dtype=dtype)
    U[..., 0:H, 0:W] = x
    S = fft2u(U) * fft2u(K) * dx * dy
    return (ifft2u(S) * (1.0 / (Ph * Pw)))[..., H:, W:]


def rsc_adjoint_from_table(g, K, dx, dy, H, W, dtype=C128):
    """g [B,C,Ph-H,Pw-W] -> [B,C,H,W]: window^T -> FFT -> conj(fft2 K) dx dy -> IFFT -> embed^T, the
    adjoint of rsc_from_table (ifft2 = F^H / N, so its adjoint is F / N and the 1 / N moves onto the
    closing inverse transform)."""
    g, K = g.to(dtype), K.to(dtype)
    B, C = g.shape[:2]
    Ph, Pw = K.shape[-2:]
    G = torch.zeros((B, C, Ph, Pw), dtype=dtype)
    G[..., H:, W:] = g
    S = fft2u(G) * fft2u(K).conj() * dx * dy
    return (ifft2u(S) * (1.0 / (Ph * Pw)))[..., 0:H, 0:W]


def vrs_from_table(x, K, dx, dy, z, dtype=C128):
    """x [2,C,H,W] (the Ex and Ey planes) -> [3,C,Ph-H,Pw-W]: Ez = Ex X / r + Ey Y / r on the unpadded
    grid linspace(-N dx / 2, N dx / 2, N) of both axes (dx on both), r = sqrt(X^2 + Y^2 + z^2), then
    the scalar convolution per component -- as tests/test_rsc_zx_gpu._oracle_planes forms it."""
    x = x.to(dtype)
    H, W = x.shape[-2:]
    X, Y, rr = _vrs_grid(H, W, dx, z, _real(dtype))
    v = torch.cat([x[0:1], x[1:2], x[0:1] * X / rr + x[1:2] * Y / rr], 0)
    return rsc_from_table(v, K, dx, dy, dtype=dtype)


def _vrs_grid(H, W, dx, z, rdt):
    xs = torch.linspace(-H * dx / 2, H * dx / 2, H, dtype=rdt)
    ys = torch.linspace(-W * dx / 2, W * dx / 2, W, dtype=rdt)
    X, Y = torch.meshgrid(xs, ys, indexing="ij")
    return X, Y, torch.sqrt(X ** 2 + Y ** 2 + torch.tensor(z, dtype=rdt) ** 2)


def vrs_adjoint_from_table(g, K, dx, dy, z, H, W, dtype=C128):
    """g [3,C,Ph-H,Pw-W] -> [2,C,H,W]: the adjoint of vrs_from_table, dEx = A^H g0 + (X / r) A^H g2 and
    dEy = A^H g1 + (Y / r) A^H g2 with A^H the scalar adjoint (the Ez weights are real)."""
    adj = rsc_adjoint_from_table(g, K, dx, dy, H, W, dtype=dtype)
    X, Y, rr = _vrs_grid(H, W, dx, z, _real(dtype))
    return torch.stack([adj[0] + adj[2] * X / rr, adj[1] + adj[2] * Y / rr])


# ---------------------------------------------------------------------------------------------
# metrics and the fp32 floor
# ---------------------------------------------------------------------------------------------
def errors(got, ref):
    """(relative L2, max|err| / rms(ref)) of ``got`` against ``ref``, both taken in complex128.  The
    second is elementwise: one wrong element of n carries 1 / sqrt(n) of a relative L2 and all of
    this one."""
    got, ref = got.to(C128), ref.to(C128)
    err = (got - ref).abs()
    rms = float(ref.abs().pow(2).mean().sqrt())
    return float(err.pow(2).sum().sqrt() / ref.abs().pow(2).sum().sqrt()), float(err.max()) / rms


def floor_of(lo, ref):
    """errors() of a complex64 run ``lo`` of the algebra against its complex128 run ``ref``, checked to
    be what a bound may rest on: an fp32 FFT pipeline is no better than one rounding (2^-24) and a few
    tens of them at the very most for transforms of up to 2^28 points."""
    rel, mx = errors(lo, ref)
    assert 2.0 ** -24 <= rel <= 2e-6 and rel <= mx <= 2e-5, f"floor32 {rel:.3e} {mx:.3e} is not an fp32 FFT's error"
    return rel, mx


def floor32(fn, *args, ref=None, **kw):
    """``fn``'s algebra in complex64 with torch's CPU FFT on the same table and input, against its
    complex128 result: (rel-L2, max|err| / rms(ref)).  ``ref``: that complex128 result, when the caller
    already holds it."""
    if ref is None:
        ref = fn(*args, dtype=C128, **kw)
    return floor_of(fn(*args, dtype=torch.complex64, **kw), ref)
