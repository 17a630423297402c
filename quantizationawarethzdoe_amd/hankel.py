"""The Hankel propagator of rotationally symmetric fields, a module of this port alone like ifta.py and tolerance.py
(csrc/thz_hankel.hip): a radial profile on the
quasi-discrete Hankel transform's nodes is carried to Z planes by two dense products with one table on the fp32
matrix cores.  The model is stated in include/thzdoe.h.
"""
import torch

from . import _lib
from ._call import _fptr, _require_device, call, workspace

_TABLES = {}  # (N, device index) -> (T, w, zeros): what the kernels use, exported once


def hankel_table(N, device):
    """(T float32 [N, N], w float32 [N], zeros float64 [N + 1]) as the kernels hold them on ``device``
    (thz_hankel_table).  The first call for an N builds the table on the host -- about N^2 / 2 evaluations of J0 in
    extended precision, a blocking step -- and every later call, of the propagator too, only launches."""
    N = int(N)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"hankel_table: the MI355X path needs a ROCm device (got device {device}); "
                           "this framework has no CPU compute path")
    key = (N, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _TABLES:
        if not 1 <= N <= _lib.HANKEL_MAX_N:
            raise ValueError(f"hankel_table: N = {N} outside 1 .. {_lib.HANKEL_MAX_N}")
        T = torch.empty(N, N, dtype=torch.float32, device=device)
        w = torch.empty(N, dtype=torch.float32, device=device)
        zeros = torch.empty(N + 1, dtype=torch.float64, device=device)
        call(_lib.lib().thz_hankel_table, N, T, w, zeros, device=device)
        _TABLES[key] = (T, w, zeros)
    return _TABLES[key]


def hankel_nodes(N, r_max, device):
    """(r, kappa, w) of N rings on the aperture radius ``r_max``: the nodes r_n = j_n r_max / S and the radial
    frequencies kappa_m = j_m / r_max in float64, and the weights w_n = 1 / |J1(j_n)| in float32 as the kernels
    use them (j: the zeros of J0, S = j_{N+1})."""
    _, w, zeros = hankel_table(N, device)
    r_max = float(r_max)
    if not r_max > 0:
        raise ValueError(f"hankel_nodes: r_max = {r_max} must be positive")
    return zeros[:-1] * r_max / zeros[-1], zeros[:-1] / r_max, w


def _desc(N, keep, Z, B, C, r_max, wavelengths, z_list):
    """HankelDesc; ``z_list``: a sequence of floats, or a float32 device tensor [Z] that the kernels read when they
    run (a captured graph then follows the tensor's values)."""
    wl = _lib.float_array(wavelengths)
    d = _lib.HankelDesc(N=N, keep=keep, Z=Z, B=B, C=C, r_max=r_max, wavelengths=_fptr(wl))
    if torch.is_tensor(z_list):
        d.z_dev = z_list.data_ptr()
        d._keep = (wl, z_list)
    else:
        zs = _lib.float_array(z_list)
        d.z = _fptr(zs)
        d._keep = (wl, zs)
    return d


def _z_arg(z_list, device, who):
    if torch.is_tensor(z_list):
        if z_list.dtype != torch.float32 or z_list.dim() != 1 or z_list.device != device:
            raise TypeError(f"{who}: a z tensor is float32 [Z] on the profile's device")
        return z_list.contiguous(), int(z_list.numel())
    zs = tuple(float(z) for z in z_list)
    return zs, len(zs)


def hankel_transfer_function(wavelengths, r_max, z_list, N, device):
    """H complex64 [Z, C, N] as the kernels form it (thz_hankel_transfer_function): exp(i z sqrt(k_c^2 - kappa_m^2))
    where kappa_m < k_c and 0 elsewhere, the phase in fp64."""
    device = torch.device(device)
    hankel_table(N, device)
    wl = tuple(float(v) for v in wavelengths)
    z, Z = _z_arg(z_list, device, "hankel_transfer_function")
    out = torch.empty(Z, len(wl), int(N), dtype=torch.complex64, device=device)
    call(_lib.lib().thz_hankel_transfer_function, _desc(int(N), int(N), Z, 1, len(wl), float(r_max), wl, z), out,
         device=device)
    return out


class _HankelPropagate(torch.autograd.Function):
    """out [Z, B, C, keep] of thz_hankel_forward; the backward is thz_hankel_adjoint.  args = (keep, r_max,
    wavelengths, z)."""

    @staticmethod
    def forward(ctx, profile, args):
        keep, r_max, wl, z = args
        profile = profile.contiguous()
        B, C, N = profile.shape
        Z = z.numel() if torch.is_tensor(z) else len(z)
        d = _desc(N, keep, Z, B, C, r_max, wl, z)
        out = torch.empty(Z, B, C, keep, dtype=torch.complex64, device=profile.device)
        ws = workspace(_lib.lib().thz_hankel_workspace_size, d, device=profile.device)
        call(_lib.lib().thz_hankel_forward, d, profile, out, ws, ws.numel(), device=profile.device)
        ctx.cfg = (args, (B, C, N, Z))
        return out

    @staticmethod
    def backward(ctx, g):
        (keep, r_max, wl, z), (B, C, N, Z) = ctx.cfg
        d = _desc(N, keep, Z, B, C, r_max, wl, z)
        g = g.contiguous()
        gp = torch.empty(B, C, N, dtype=torch.complex64, device=g.device)
        ws = workspace(_lib.lib().thz_hankel_workspace_size, d, device=g.device)
        call(_lib.lib().thz_hankel_adjoint, d, g, gp, ws, ws.numel(), device=g.device)
        return gp, None


def hankel_propagate(profile, wavelengths, r_max, z_list, keep=None):
    """A rotationally symmetric field on Z planes: ``profile`` complex64 [B, C, N], the field at the N nodes of
    ``hankel_nodes(N, r_max)``, -> complex64 [Z, B, C, keep], the field at the first ``keep`` nodes (default N) of
    every plane of ``z_list`` (thz_hankel_forward: the angular-spectrum method in the radial coordinate, ASM_prop's
    evanescent rule and sign; the model is in include/thzdoe.h).

    The field vanishes at r = r_max, the transform's boundary: choose ``r_max`` larger than the element, as
    ``padding_scale`` does for the 2-D propagators.  ``z_list``: floats, or a float32 device tensor [Z] read when
    the kernels run.  Gradients flow to ``profile`` (thz_hankel_adjoint); none to z or r_max.

    The first call for an N on a device builds the library's table on the host (about N^2 / 2 values of J0 in
    extended precision, 0.4 s at N = 4096) and copies it: that call blocks and cannot be captured.  Every later call
    has no host sync and is capturable in torch.cuda.graph.  A repeated call gives the same bits.  Z planes of one
    call equal Z one-plane calls, and ``keep`` < N the first ``keep`` entries of ``keep`` = N, bit for bit where both
    calls split K alike -- always for N <= 128 -- and to rounding otherwise: the number of K ranges follows the
    shape (include/thzdoe.h)."""
    who = "hankel_propagate"
    if not torch.is_tensor(profile):
        raise TypeError(f"{who}: profile must be a tensor")
    _require_device(profile, who)
    if profile.dtype == torch.complex128:
        raise TypeError(f"{who}: the kernels compute in complex64; got a complex128 profile -- cast it, an fp64 "
                        "variant does not exist")
    if profile.dtype != torch.complex64 or profile.dim() != 3:
        raise TypeError(f"{who}: profile is complex64 [B, C, N]; got {profile.dtype} {tuple(profile.shape)}")
    B, C, N = profile.shape
    wl = tuple(float(v) for v in wavelengths)
    if len(wl) != C:
        raise ValueError(f"{who}: {len(wl)} wavelengths for a profile of {C} channels")
    keep = N if keep is None else int(keep)
    z, _ = _z_arg(z_list, profile.device, who)
    return _HankelPropagate.apply(profile, (keep, float(r_max), wl, z))
