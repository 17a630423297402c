"""Thick-element DOE: split-step (multi-slice) propagation through the relief on fused kernels, forward and native
backward (csrc/thz_thick.hip).
"""
import numpy as np
import torch

from .. import _lib, doe, propagation
from .._call import _fptr, _launch, _require_device

THICK_CONVENTIONS = {"reference": -1.0, "physical": 1.0}
_THICK_MAX_SLICES = 256
_THICK_BASE_PLANE = float(np.float32(2e-3))  # DOE_BASE_PLANE (csrc/thz_dev.hpp), BASE_PLANE_THICKNESS of the layers


def thick_doe_native(H, W, pad_h, pad_w, slices):
    """True where thz_thick_forward serves the geometry: padded sides that are powers of two from 64 to
    8192 (they may differ) and at most 256 slices."""
    def pow2(n):
        return 64 <= n <= 8192 and n & (n - 1) == 0
    return pow2(H + 2 * pad_h) and pow2(W + 2 * pad_w) and slices <= _THICK_MAX_SLICES


def _thick_desc(field, height, wavelengths, spacing, eps, tand, thickness, slices, pad_h, pad_w, bl, sign):
    B, C, H, W = field.shape
    wl = _lib.float_array(wavelengths)
    d = _lib.ThickDesc(B=B, C=C, H=H, W=W, pad_h=pad_h, pad_w=pad_w, bandlimit=bl, hs=height.shape[0],
                       ws=height.shape[1], slices=slices, thickness=thickness, dx=float(spacing[0]),
                       dy=float(spacing[1]), epsilon=float(eps), tand=float(tand), phase_sign=sign,
                       wavelengths=_fptr(wl))
    d._keep = wl
    return d


def _thick_fused(field, height, *args, stash=None):
    """thz_thick_forward, or thz_thick_forward_saved into ``stash`` [B, C, H, W] complex64."""
    d = _thick_desc(field, height, *args)
    out = torch.empty_like(field)
    L = _lib.lib()
    if stash is None:
        _launch(L.thz_thick_workspace_size, L.thz_thick_forward, d, field.device, field, height, out)
    else:
        _launch(L.thz_thick_workspace_size, L.thz_thick_forward_saved, d, field.device, field, height, out, stash)
    return out


class _ThickFused(torch.autograd.Function):
    """thick_doe(grad="fused"): the fused forward (the saving one when the map requires grad) and
    thz_thick_backward, which forms no slab field and keeps one stash: V_s where slab s is the pixel's active one."""

    @staticmethod
    def forward(ctx, field, height, args):
        x, h = field.detach().resolve_conj().contiguous(), height.detach().contiguous()  # the kernels read memory
        need_h = ctx.needs_input_grad[1]
        stash = torch.empty_like(x) if need_h else None
        out = _thick_fused(x, h, *args, stash=stash)
        ctx.args, ctx.shape = args, tuple(x.shape)
        ctx.save_for_backward(h, stash)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        h, stash = ctx.saved_tensors
        need_x, need_h = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_x or need_h):
            return None, None, None
        g = grad_out.resolve_conj().contiguous()
        if g.dtype != torch.complex64:
            raise TypeError(f"thick_doe backward: grad_out must be complex64; got {g.dtype}")
        d = _thick_desc(g, h, *ctx.args)
        gx = torch.empty_like(g) if need_x else None
        gh = torch.empty_like(h) if need_h else None
        L = _lib.lib()
        _launch(L.thz_thick_backward_workspace_size, L.thz_thick_backward, d, g.device, g, h, stash, gx, gh)
        return gx, gh, None


def _thick_compose(field, height, wavelengths, spacing, eps, tand, thickness, slices, pad_h, pad_w, bl, sign):
    dz = float(np.float32(thickness)) / slices  # the library's dz: the fp32 thickness over S, in double
    u = field
    for s in range(slices):
        d = (height - s * dz).clamp(0.0, dz)
        if s > 0:
            d = d - _THICK_BASE_PLANE  # the modulate kernel adds the base plate to its argument
        # sign = +1: U conj(t) = conj(conj(U) t); the kernels read memory, so the conjugates are formed
        u = doe.modulate(u.conj().resolve_conj() if sign > 0 else u, d, wavelengths, eps, tand)[0]
        u = propagation.asm_propagate(u.conj().resolve_conj() if sign > 0 else u, wavelengths, spacing, [dz], pad_h,
                                      pad_w, True, bl)[0]
    return u


def thick_doe(field, height, wavelengths, spacing, eps, tand, thickness, slices, padding_scale=1, bandlimit="exact",
              convention="reference", method="auto", grad=None):
    """The field behind a DOE of finite thickness: split-step (multi-slice) propagation through the relief.

    ``field`` complex64 [B, C, H, W]; ``height`` float32 [hs, ws], nearest-upsampled to [H, W]; ``thickness`` T
    > 0 and ``slices`` S >= 1.  With dz = T / S and d_s = clamp(h - s dz, 0, dz) (d_0 also carries the base
    plate), slab s multiplies by t_s = exp(-k/2 d_s tand sqrt(eps)) exp(sigma i k d_s (sqrt(eps) - 1)) and
    ASM_prop(z_distance=dz, padding_scale, bandlimit) carries the field to the next slab, cropped every step.
    The result is the field in the plane T above the base plate; heights above T count as T, below 0 as 0.

    ``convention``: "reference" (sigma = -1, DOELayer.modulate's sign: S = 1 is modulate then ASM over T) or
    "physical" (sigma = +1, consistent with the ASM's exp(+i z k_z)).  ``bandlimit``: "exact", "approx" or None.
    ``method``: "fused" -- the thz_thick.hip kernels, two launches per slab, capturable, forward only unless
    ``grad`` says otherwise; padded sides must be powers of two from 64 to 8192 and S <= 256.  "compose" -- the same model as a loop over doe.modulate
    and the ASM kernels, differentiable in the field and the map.  "auto": fused where it serves the geometry and
    nothing requires grad, else compose.

    ``grad``: None -- as above.  "fused" -- the gradient of the fused path is the native backward
    (thz_thick_backward): "fused" and, on a geometry the kernels serve, "auto" then stay on the fused kernels when
    something requires grad; the forward keeps one field-sized stash instead of every slab's field.  "auto" on
    another geometry falls back to compose, method="fused" there raises the library's unsupported error, and
    method="compose" with grad="fused" is a ValueError.  The derivative in a height is taken inside the slab the
    height ends in; a height exactly on a slab face, on 0 or on T, below 0 or above T has gradient 0."""
    who = "thick_doe"
    if grad not in (None, "fused"):
        raise ValueError(f"{who}: grad must be None or 'fused'; got {grad!r}")
    if grad == "fused" and method == "compose":
        raise ValueError(f"{who}: grad='fused' is the backward of the fused kernels; method='compose' has autograd's")
    _require_device(field, who)
    if field.dtype != torch.complex64:
        raise TypeError(f"{who}: the DOE kernels compute in complex64; got {field.dtype}")
    if field.dim() != 4 or height.dim() != 2:
        raise ValueError(f"{who}: field [B, C, H, W] and height [hs, ws]; got {tuple(field.shape)}, {tuple(height.shape)}")
    if convention not in THICK_CONVENTIONS:
        raise ValueError(f"{who}: convention must be 'reference' or 'physical'; got {convention!r}")
    if method not in ("auto", "fused", "compose"):
        raise ValueError(f"{who}: method must be 'auto', 'fused' or 'compose'; got {method!r}")
    slices = int(slices)
    thickness = float(np.float32(thickness))
    if slices < 1 or not thickness > 0.0:
        raise ValueError(f"{who}: thickness > 0 and slices >= 1; got {thickness}, {slices}")
    B, C, H, W = field.shape
    wavelengths = [float(w) for w in wavelengths]
    if len(wavelengths) != C:
        raise ValueError(f"{who}: {len(wavelengths)} wavelengths for {C} channels")
    spacing = (float(spacing[0]), float(spacing[1])) if np.ndim(spacing) else (float(spacing), float(spacing))
    ps = padding_scale if np.ndim(padding_scale) else (padding_scale, padding_scale)
    pad_h, pad_w = propagation.asm_padding(H, W, ps)
    bl = propagation._bandlimit(bandlimit)
    sign = THICK_CONVENTIONS[convention]
    diff = torch.is_grad_enabled() and (field.requires_grad or height.requires_grad)
    native = thick_doe_native(H, W, pad_h, pad_w, slices)
    if method == "auto":
        method = "fused" if native and (not diff or grad == "fused") else "compose"
    height = height.to(device=field.device, dtype=torch.float32)
    args = (wavelengths, spacing, float(eps), float(tand), thickness, slices, pad_h, pad_w, bl, sign)
    if method == "compose":
        return _thick_compose(field, height, *args)
    if diff and grad == "fused":
        return _ThickFused.apply(field, height, args)
    if diff:
        raise RuntimeError(f"{who}: method='fused' is forward only unless grad='fused'; use that, or method='compose' "
                           "(or 'auto'), for gradients")
    return _thick_fused(field.detach().contiguous(), height.detach().contiguous(), *args)
