"""Least-squares 2-D phase unwrapping of a field, a module of this port alone like zernike.py (csrc/thz_unwrap.hip;
DESIGN §42; the glue to the entry points lives here too, as zernike.py's does).  A complex field's wavefront is only
known modulo 2 pi; ``unwrap_phase`` returns the continuous phase that ``zernike.fit``, ``zernike.residual`` and ``metrics.wavefront_rms`` take, ``wavefront`` the optical path in
metres, ``residues`` the map of the points where no continuous phase exists.

The method is Ghiglia and Romero's: the wrapped differences of neighbouring pixels (taken from the field itself,
arg(U[j+1] conj U[j]), never from an angle map) are integrated in the least-squares sense by a Neumann Poisson
solve -- a cosine transform, division by the Laplacian's eigenvalues, and the transform back -- and, with weights
or for sides that are not powers of two, by preconditioned conjugate gradients on that solve.  The model is stated
in include/thzdoe.h (thz_unwrap_*).  Not differentiable: the weighted Laplacian is symmetric, so a backward pass
would be the same solve, but none is built.
"""
import math

import torch

from . import _lib
from ._call import _require_device, call, workspace
from .DataType.ElectricField import ElectricField

UNWRAP_WEIGHTS = {"amplitude": _lib.UNWRAP_W_AMPLITUDE, "intensity": _lib.UNWRAP_W_INTENSITY}
UNWRAP_MIN_SIDE, UNWRAP_MAX_SIDE = 64, 4096
UNWRAP_DEFAULT_ITERS = 20


def _planes(x, who):
    """(contiguous [BC, H, W] view, input kind) of a complex64 field or a float32 wrapped phase"""
    if not torch.is_tensor(x):
        raise TypeError(f"{who}: the input must be a tensor or an ElectricField")
    _require_device(x, who)
    if x.dtype not in (torch.complex64, torch.float32):
        raise TypeError(f"{who}: a complex64 field or a float32 wrapped phase; got {x.dtype} -- the kernels compute "
                        "in float32, an fp64 variant does not exist")
    if x.dim() < 2 or x.shape[-2] < 2 or x.shape[-1] < 2:
        raise ValueError(f"{who}: the input is [..., H, W] with H, W >= 2; got {tuple(x.shape)}")
    H, W = x.shape[-2:]
    if max(H, W) > UNWRAP_MAX_SIDE:
        raise ValueError(f"{who}: plane {H} x {W}; each side is at most {UNWRAP_MAX_SIDE}")
    p = x.detach().resolve_conj().contiguous().reshape(-1, H, W)
    if p.shape[0] < 1:
        raise ValueError(f"{who}: empty input {tuple(x.shape)}")
    return p, (_lib.UNWRAP_FIELD if x.is_complex() else _lib.UNWRAP_PHASE)


def direct_solvable(H, W):
    """Whether an unweighted H x W plane takes the direct solve: both sides powers of two from 64."""
    return all(n >= UNWRAP_MIN_SIDE and n & (n - 1) == 0 for n in (H, W))


def _unwrap_planes(x, weights=None, iters=None, tol=1e-6, congruent=False, anchor=None):
    """``(phi, hist)`` of thz_unwrap_phase: phi float32 shaped like ``x``, hist float64 [iters, BC] (None for the
    direct solve).  ``weights``: None, "amplitude", "intensity" or a float32 tensor [H, W] / broadcastable to the
    planes; ``anchor``: None or a pixel (row, col).  ``iters`` None: 0 where the direct solve applies, else 20."""
    who = "unwrap_phase"
    p, kind = _planes(x, who)
    BC, H, W = p.shape
    wkind, warr, wstride = _lib.UNWRAP_W_NONE, None, 0
    if isinstance(weights, str):
        if weights not in UNWRAP_WEIGHTS:
            raise ValueError(f"{who}: weights is None, 'amplitude', 'intensity' or a tensor; got {weights!r}")
        if kind == _lib.UNWRAP_PHASE:
            raise ValueError(f"{who}: {weights!r} weights need a complex field, not a phase map")
        wkind = UNWRAP_WEIGHTS[weights]
    elif weights is not None:
        if not torch.is_tensor(weights) or weights.is_complex():
            raise TypeError(f"{who}: weights is None, 'amplitude', 'intensity' or a real tensor")
        if weights.device != p.device:
            raise ValueError(f"{who}: weights on {weights.device}, the input on {p.device}")
        warr = weights.detach().to(torch.float32)
        if tuple(warr.shape[-2:]) != (H, W):
            raise ValueError(f"{who}: weights {tuple(warr.shape)} do not match the {H} x {W} planes")
        if warr.numel() == H * W:
            warr = warr.reshape(H, W).contiguous()
        else:
            warr, wstride = warr.expand(x.shape).contiguous().reshape(BC, H, W), H * W
        wkind = _lib.UNWRAP_W_ARRAY
    if iters is None:
        iters = 0 if wkind == _lib.UNWRAP_W_NONE and direct_solvable(H, W) else UNWRAP_DEFAULT_ITERS
    iters = int(iters)
    if iters < 0:
        raise ValueError(f"{who}: iters = {iters}")
    if iters == 0 and not (wkind == _lib.UNWRAP_W_NONE and direct_solvable(H, W)):
        raise ValueError(f"{who}: iters = 0 is the direct solve, which takes unweighted planes whose sides are powers "
                         f"of two from {UNWRAP_MIN_SIDE}; {H} x {W}{' with weights' if wkind else ''} needs iterations")
    if anchor is None:
        ar = ac = aon = 0
    else:
        ar, ac = (H // 2, W // 2) if isinstance(anchor, str) and anchor == "center" else (int(v) for v in anchor)
        if not (0 <= ar < H and 0 <= ac < W):
            raise ValueError(f"{who}: anchor ({ar}, {ac}) outside the {H} x {W} plane")
        aon = 1
    d = _lib.UnwrapDesc(BC=BC, H=H, W=W, input=kind, weights=wkind, iters=iters, wstride=wstride, tol=float(tol),
                        anchor=aon, anchor_row=ar, anchor_col=ac, congruent=int(bool(congruent)))
    out = torch.empty((BC, H, W), dtype=torch.float32, device=p.device)
    hist = torch.empty((iters, BC), dtype=torch.float64, device=p.device) if iters else None
    ws = workspace(_lib.lib().thz_unwrap_workspace_size, d, device=p.device)
    call(_lib.lib().thz_unwrap_phase, d, p, warr, out, hist, ws, ws.numel(), device=p.device)
    return out.reshape(x.shape), hist


def _residue_map(x):
    """int8 [..., H - 1, W - 1]: the charge of every 2 x 2 loop of a complex64 field or float32 wrapped phase."""
    p, kind = _planes(x, "residues")
    BC, H, W = p.shape
    out = torch.empty((BC, H - 1, W - 1), dtype=torch.int8, device=p.device)
    call(_lib.lib().thz_unwrap_residues, BC, H, W, kind, p, out, device=p.device)
    return out.reshape(tuple(x.shape[:-2]) + (H - 1, W - 1))


def _data(field):
    return field.data if isinstance(field, ElectricField) else field


def unwrap_phase(field, weights=None, iters=None, tol=1e-6, congruent=False, anchor="center", return_history=False):
    """The unwrapped phase of ``field``, float32 with the input's shape.

    ``field``: an ElectricField, a complex64 tensor [..., H, W] or a float32 wrapped phase map, on the ROCm device;
    H, W from 2 to 4096.  ``weights``: None (w = 1), "amplitude" (|U| / max |U| of each plane), "intensity"
    (|U|^2 / max) or a float32 tensor [H, W] / broadcastable to the planes with values in [0, 1]; a pixel of
    weight 0 (a hole, a dead detector pixel, the outside of a pupil) does not take part and may hold anything.
    Unweighted planes whose sides are powers of two from 64 take the direct solve; everything else runs ``iters``
    (default 20) conjugate-gradient steps, each preconditioned by the direct solve, and a step is frozen on the
    device once the residual has fallen by ``tol``.  ``anchor``: "center" shifts the result so that pixel
    (H // 2, W // 2) equals arg U there, (row, col) anchors at that pixel, None keeps the raw (zero-mean for the
    direct solve) solution.  ``congruent``: return arg U + 2 pi k with the integer map k nearest to the solution --
    exact wherever the field has no residues.  ``return_history``: also return sqrt(rz_k / rz_0), float64
    [iters, planes] (None for the direct solve).  No host sync; capturable in torch.cuda.graph after a first call
    at the same sizes."""
    phi, hist = _unwrap_planes(_data(field), weights=weights, iters=iters, tol=tol, congruent=congruent,
                                anchor=anchor)
    return (phi, hist) if return_history else phi


def wavefront(field, wavelengths=None, **kwargs):
    """The optical path ``unwrap_phase(field, **kwargs) lambda_c / (2 pi)`` in metres, per channel: ``field`` is an
    ElectricField, or a complex64 [B, C, H, W] tensor with ``wavelengths`` (C values, metres)."""
    if wavelengths is None:
        if not isinstance(field, ElectricField):
            raise TypeError("wavefront: a tensor needs its wavelengths")
        wavelengths = field.wavelengths_host
    lam = torch.as_tensor(wavelengths, dtype=torch.float64).reshape(-1)
    phi = unwrap_phase(field, **kwargs)
    if phi.dim() != 4 or phi.shape[1] != lam.numel():
        raise ValueError(f"wavefront: field {tuple(phi.shape)} is not [B, C, H, W] with C = {lam.numel()} wavelengths")
    return phi * (lam / (2 * math.pi)).to(device=phi.device, dtype=torch.float32).reshape(1, -1, 1, 1)


def residues(field):
    """int8 [..., H - 1, W - 1]: +1 / -1 / 0, the wrapped differences summed round every 2 x 2 loop of pixels in
    units of 2 pi.  Where it is not 0 a least-squares solution cannot be congruent with the field."""
    return _residue_map(_data(field))
