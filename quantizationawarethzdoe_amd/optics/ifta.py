"""The IFTA / Gerchberg-Saxton projections behind ifta.py: target statistics, target projection and the DOE
projection onto the level table (csrc/thz_ifta.hip).
"""
import torch

from .. import _lib
from .._call import _require_device, call, workspace
from .heightmap import as_planes, host_table

IFTA_STATS = ("S_all", "S_in", "S_TU", "S_TT", "s", "eff")  # the columns of ifta_target_stats


def _ifta_planes(U, who):
    """The field as contiguous [N, H, W] complex64 planes on the device."""
    if not torch.is_tensor(U):
        raise TypeError(f"{who}: the field must be a tensor")
    _require_device(U, who)
    if U.dtype == torch.complex128:
        raise TypeError(f"{who}: the IFTA kernels compute in complex64; got a complex128 field -- cast it to "
                        "complex64")
    if U.dtype != torch.complex64:
        raise TypeError(f"{who}: a complex64 field; got {U.dtype}")
    return as_planes(U.resolve_conj().contiguous(), who)


def _ifta_target(T, mask, planes, who):
    """(T float32 contiguous, its plane count 1 or N, mask uint8 [H, W] or None) for [N, H, W] planes."""
    N, H, W = planes.shape
    if not torch.is_tensor(T) or T.is_complex() or T.device != planes.device:
        raise TypeError(f"{who}: the target amplitude must be a real tensor on {planes.device}")
    if T.dim() < 2 or tuple(T.shape[-2:]) != (H, W) or T.numel() not in (H * W, N * H * W):
        raise ValueError(f"{who}: target {tuple(T.shape)} for planes {(N, H, W)}: [H, W] or one per plane")
    T = T.detach().to(torch.float32).contiguous()
    if mask is not None:
        if not torch.is_tensor(mask) or mask.device != planes.device or mask.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"{who}: the window mask must be a bool / uint8 tensor on {planes.device}")
        if tuple(mask.shape) != (H, W):
            raise ValueError(f"{who}: window mask {tuple(mask.shape)} for planes of {(H, W)}")
        mask = mask.contiguous()
        mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    return T, (1 if T.numel() == H * W else N), mask


def ifta_target_stats(U, T, mask=None, out=None):
    """The sums one IFTA iteration needs of the planes ``U`` against the target amplitude ``T``, in one pass
    (thz_ifta_target_stats).

    ``U``: complex64 [..., H, W] on the ROCm device (N planes).  ``T``: real, [H, W] for every plane or one per
    plane, non-negative.  ``mask``: bool / uint8 [H, W], the signal window; None: every pixel.  Returns float64
    [N, 6] = (S_all = sum |U|^2, S_in = sum_M |U|^2, S_TU = sum_M T |U|, S_TT = sum_M T^2, s = S_TU / S_TT,
    eff = S_in / S_all), quotients 0 where the denominator is 0; ``s`` is the least-squares scale of s T against
    |U| on the window.  ``out``: a contiguous float64 [N, 6] device tensor (a row of a history array) to write
    instead.  Sums are float64 in a fixed order: the same input gives the same bits.  No autograd, no host sync;
    capturable in torch.cuda.graph."""
    who = "ifta_target_stats"
    p = _ifta_planes(U, who)
    T, tp, mask = _ifta_target(T, mask, p, who)
    N, H, W = p.shape
    if out is None:
        out = torch.empty((N, 6), dtype=torch.float64, device=p.device)
    elif (not torch.is_tensor(out) or out.dtype != torch.float64 or out.device != p.device or not out.is_contiguous()
          or tuple(out.shape) != (N, 6)):
        raise ValueError(f"{who}: out must be a contiguous float64 [{N}, 6] tensor on {p.device}")
    d = _lib.IftaDesc(N=N, H=H, W=W, target_planes=tp, alpha=1.0, beta=1.0)
    ws = workspace(_lib.lib().thz_ifta_target_stats_workspace_size, d, device=p.device)
    call(_lib.lib().thz_ifta_target_stats, d, p, T, mask, out, ws, ws.numel(), device=p.device)
    return out


def ifta_target_project(U, T, scale, mask=None, alpha=1.0, beta=1.0, out=None):
    """Impose the target amplitude on the planes ``U`` (thz_ifta_target_project): inside the window
    a' = max(0, alpha s T + (1 - alpha) |U|) with U's phase (a' itself where U = 0), outside it beta U.

    ``U``, ``T``, ``mask`` as ``ifta_target_stats``.  ``scale``: float64 device tensor, one value per plane
    (column ``s`` of the stats, or a joint scale), read by the kernel.  ``alpha`` in (0, 2]: 1 is
    Gerchberg-Saxton, above 1 the over-compensated form; ``beta`` in [0, 1]: 1 leaves the amplitude outside the
    window free, 0 suppresses it.  ``out``: a contiguous complex64 tensor of U's shape; ``out=U`` projects in
    place.  Returns the projected planes in U's shape.  No autograd, no host sync; capturable."""
    who = "ifta_target_project"
    alpha, beta = float(alpha), float(beta)
    if not 0.0 < alpha <= 2.0:
        raise ValueError(f"{who}: alpha must lie in (0, 2]; got {alpha}")
    if not 0.0 <= beta <= 1.0:
        raise ValueError(f"{who}: beta must lie in [0, 1]; got {beta}")
    if out is not None and out is U and not U.is_contiguous():
        raise ValueError(f"{who}: in place needs a contiguous field")
    p = _ifta_planes(U, who)
    T, tp, mask = _ifta_target(T, mask, p, who)
    N, H, W = p.shape
    if (not torch.is_tensor(scale) or scale.dtype != torch.float64 or scale.device != p.device
            or scale.numel() != N):
        raise ValueError(f"{who}: scale must be a float64 tensor of {N} values on {p.device}")
    scale = scale.detach().reshape(-1).contiguous()
    if out is None:
        out = torch.empty_like(p)
    elif (not torch.is_tensor(out) or out.dtype != torch.complex64 or out.device != p.device
          or not out.is_contiguous() or out.numel() != p.numel()):
        raise ValueError(f"{who}: out must be a contiguous complex64 tensor of {tuple(U.shape)} on {p.device}")
    d = _lib.IftaDesc(N=N, H=H, W=W, target_planes=tp, alpha=alpha, beta=beta)
    call(_lib.lib().thz_ifta_target_project, d, p, T, mask, scale, out, device=p.device)
    return out.reshape(U.shape)


def ifta_doe_desc(N, H, W, doe_shape, wavelength, eps, lut, incident_planes, who="ifta_doe_project"):
    hs, ws = int(doe_shape[0]), int(doe_shape[1])
    if hs < 1 or ws < 1 or H % hs or W % ws:
        raise ValueError(f"{who}: a {H} x {W} field over {hs} x {ws} cells: every cell must be a whole number of "
                         "field pixels")
    if not 1 <= len(lut) <= _lib.THZ_MAX_LUT:
        raise ValueError(f"{who}: {len(lut)} levels; the kernels take 1 .. {_lib.THZ_MAX_LUT}")
    d = _lib.IftaDoeDesc(N=N, H=H, W=W, hs=hs, ws=ws, incident_planes=incident_planes, wavelength=float(wavelength),
                         epsilon=float(eps), L=len(lut))
    for i, v in enumerate(lut):
        d.lut[i] = v
    return d


def ifta_doe_project(U, doe_shape, wavelength, eps, lut, q=1.0, incident=None):
    """Turn the back-propagated field ``U`` into a height map on the level table (thz_ifta_doe_project).

    ``U``: complex64 [..., H, W] (N fields); ``doe_shape`` = (hs, ws) cells, each a whole number r_h x r_w of
    field pixels.  ``incident``: the field A that lit the DOE, complex64 [H, W] or one per field; None: 1.  Per
    cell g = sum U conj(A) (float64, row-major), h_c = (-arg g / kappa - base plane) mod h_max with kappa =
    2 pi / wavelength (sqrt(eps) - 1) and h_max = 2 pi / kappa, then the nearest level of ``lut`` (ascending in
    [0, h_max)) on the circle, the lowest index on a tie; the cell takes it when its cyclic distance is at most
    ``q`` times half the gap to the neighbouring level on its side, and keeps h_c otherwise.  ``q`` in [0, 1]: a
    Python number, or a float32 device tensor [1] the kernel reads when it runs (a captured graph sees each
    replay's value); 0 leaves the map continuous, 1 snaps every cell.  ``lut``: a list or CPU tensor; a device
    tensor is read back on every call and refused during a graph capture, as ``lut_quantize`` does.  The loss
    tangent takes no part.

    Returns ``(h, idx)``: float32 and int32 [..., hs, ws]; idx is the level, -1 where the cell kept h_c.  No
    autograd, no host sync with a host table; capturable."""
    who = "ifta_doe_project"
    p = _ifta_planes(U, who)
    N, H, W = p.shape
    lut = host_table(lut, who, torch.float32)
    planes = 0
    if incident is not None:
        if not torch.is_tensor(incident) or incident.device != p.device:
            raise TypeError(f"{who}: the incident field must be a tensor on {p.device}")
        if incident.dtype != torch.complex64:
            raise TypeError(f"{who}: the IFTA kernels compute in complex64; got an incident field of {incident.dtype}")
        if incident.dim() < 2 or tuple(incident.shape[-2:]) != (H, W) or incident.numel() not in (H * W, N * H * W):
            raise ValueError(f"{who}: incident field {tuple(incident.shape)} for {(N, H, W)}: [H, W] or one per field")
        incident = incident.detach().resolve_conj().contiguous()
        planes = 1 if incident.numel() == H * W else N
    d = ifta_doe_desc(N, H, W, doe_shape, wavelength, eps, lut, planes, who)
    if torch.is_tensor(q):
        if not q.is_cuda or q.dtype != torch.float32 or q.numel() != 1 or q.device != p.device:
            raise ValueError(f"{who}: q as a tensor must be one float32 value on {p.device}")
        q_dev = q.detach()
    else:
        if not 0.0 <= float(q) <= 1.0:
            raise ValueError(f"{who}: q must lie in [0, 1]; got {q}")
        q_dev = torch.full((1,), float(q), dtype=torch.float32, device=p.device)
    lead = tuple(U.shape[:-2])
    h = torch.empty(lead + (d.hs, d.ws), dtype=torch.float32, device=p.device)
    idx = torch.empty(lead + (d.hs, d.ws), dtype=torch.int32, device=p.device)
    call(_lib.lib().thz_ifta_doe_project, d, p, incident, q_dev, h, idx, device=p.device)
    return h, idx
