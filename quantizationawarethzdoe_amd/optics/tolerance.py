"""The fabrication-tolerance screen behind tolerance.py: K perturbed realisations of a height map applied to a
field in one streaming pass (csrc/thz_tolerance.hip).
"""
import ctypes
import math

import torch

from .. import _lib
from .._call import _fptr, _require_device, call
from .noise import noise_state

TOLERANCE_ROUGHNESS = {"uniform": _lib.TOL_ROUGH_UNIFORM, "normal": _lib.TOL_ROUGH_NORMAL}


def tolerance_cfg(fab, who):
    """(sigma_scale, level table, roughness code, roughness, lo, hi) of a ``tolerance.FabricationModel`` (or
    anything with its four attributes); a scalar ``sigma_level`` other than 0 serves every level index."""
    levels = fab.sigma_level
    if isinstance(levels, (int, float)):
        levels = (float(levels),) * _lib.THZ_MAX_LUT if float(levels) != 0.0 else ()
    levels = tuple(float(v) for v in levels)
    if len(levels) > _lib.THZ_MAX_LUT:
        raise ValueError(f"{who}: {len(levels)} level sigmas; the kernel takes up to {_lib.THZ_MAX_LUT}")
    code, rough = _lib.TOL_ROUGH_NONE, 0.0
    if fab.roughness is not None:
        name, rough = fab.roughness
        if name not in TOLERANCE_ROUGHNESS:
            raise ValueError(f"{who}: roughness must be None, ('uniform', a) or ('normal', s); got {fab.roughness!r}")
        code, rough = TOLERANCE_ROUGHNESS[name], float(rough)
    lo, hi = fab.clamp
    return (float(fab.sigma_scale), levels, code, rough, -math.inf if lo is None else float(lo),
            math.inf if hi is None else float(hi))


def _tolerance_desc(cfg, K, first, field, height, eps, tand, wavelengths, state, stream):
    sigma_scale, levels, code, rough, lo, hi = cfg
    Bf, C, H, W = field.shape
    wl = _lib.float_array(wavelengths)
    d = _lib.ToleranceDesc(K=K, first=first, Bf=Bf, C=C, H=H, W=W, hs=height.shape[0], ws=height.shape[1],
                           L=len(levels), sigma_level=(ctypes.c_float * _lib.THZ_MAX_LUT)(*levels),
                           sigma_scale=sigma_scale, rough_kind=code, rough=rough, lo=lo, hi=hi,
                           epsilon=eps, tand=tand, wavelengths=_fptr(wl), rng=state.data_ptr(), stream=stream)
    d._keep = wl
    return d


class _ToleranceModulate(torch.autograd.Function):
    """out [K, C, H, W] (and the realised maps [K, hs, ws]) of thz_tolerance_modulate_forward.  args = (K, first,
    stream, eps, tand, wavelengths, cfg, want_heights)."""

    @staticmethod
    def forward(ctx, field, height, idx, state, args):
        K, first, stream, eps, tand, wavelengths, cfg, want_heights = args
        field, height = field.contiguous(), height.detach().contiguous()
        d = _tolerance_desc(cfg, K, first, field, height, eps, tand, wavelengths, state, stream)
        out = torch.empty((K,) + tuple(field.shape[1:]), dtype=torch.complex64, device=field.device)
        heights = torch.empty((K,) + tuple(height.shape), dtype=torch.float32, device=field.device) if want_heights else None
        call(_lib.lib().thz_tolerance_modulate_forward, d, field, height, idx, out, heights, device=field.device)
        ctx.save_for_backward(field, height, idx, state)
        ctx.args = args
        if heights is not None:
            ctx.mark_non_differentiable(heights)
        return out, heights

    @staticmethod
    def backward(ctx, g, _gh):
        field, height, idx, state = ctx.saved_tensors
        K, first, stream, eps, tand, wavelengths, cfg, _ = ctx.args
        d = _tolerance_desc(cfg, K, first, field, height, eps, tand, wavelengths, state, stream)
        g = g.contiguous()
        gf = torch.empty_like(field) if ctx.needs_input_grad[0] else None
        gh = torch.empty_like(height) if ctx.needs_input_grad[1] else None
        call(_lib.lib().thz_tolerance_modulate_backward, d, g, field, height, idx, gf, gh, None, 0, device=field.device)
        return gf, gh, None, None, None


def tolerance_modulate(field, height, wavelengths, eps, tand, fab, K, *, idx=None, rng=None, first=0,
                       return_heights=False):
    """K fabrication-perturbed realisations of the height map ``height`` applied to ``field`` in one streaming
    pass (thz_tolerance_modulate_forward): ``out[k] = field[b] * t(h_k)`` with, for realisation ``first + k``,

        h_k = clamp((1 + g_k) h + e_{k, idx} + r_k, lo, hi)

    -- a depth-scale error g_k = sigma_scale n, a depth error per level e_{k,l} = sigma_level[l] n (``idx`` [hs,
    ws] gives every map pixel's level, e.g. from ``lut_quantize(h, lut, mode="argmin")``; a value outside the
    table takes none) and a per-pixel roughness r_k (the reference's ``(u - 0.5) 2 a`` or ``s n``), as
    ``fab``, a ``tolerance.FabricationModel``, states them.

    ``field``: complex64 [1, C, H, W] (one incident field for every realisation) or [K, C, H, W]; ``height``:
    float32 [hs, ws], upsampled to the field by the nearest rule of ``doe.modulate``.  Returns ``out`` [K, C, H,
    W], and ``(out, heights)`` with the realised maps [K, hs, ws] when ``return_heights``; ``out[k]`` equals
    ``doe.modulate(field, heights[k])`` bit for bit.

    ``rng = (state, stream)`` as in ``add_noise`` (None: a state drawn on the device from torch's generator).
    Realisation k is a pure function of (state, stream, k): chunks of a run (``first`` advancing) give the bits
    of one call.  Gradients flow to ``height`` and ``field`` (thz_tolerance_modulate_backward: every draw
    regenerated, fp64 sums in a fixed order, no atomics), which makes the mean of a loss over the K outputs
    a robust-design objective.  No host sync; capturable in torch.cuda.graph."""
    who = "tolerance_modulate"
    if not torch.is_tensor(field) or not torch.is_tensor(height):
        raise TypeError(f"{who}: field and height must be tensors")
    _require_device(field, who)
    _require_device(height, who)
    if field.dtype != torch.complex64 or height.dtype != torch.float32:
        raise TypeError(f"{who}: the kernel computes in complex64 / float32; got {field.dtype} and {height.dtype}")
    K, first = int(K), int(first)
    if K < 1 or first < 0:
        raise ValueError(f"{who}: K = {K} must be >= 1 and first = {first} >= 0")
    if field.dim() != 4 or field.shape[0] not in (1, K):
        raise ValueError(f"{who}: the field must be [1, C, H, W] or [K = {K}, C, H, W]; got {tuple(field.shape)}")
    if height.dim() != 2:
        raise ValueError(f"{who}: one height map [hs, ws]; got {tuple(height.shape)}")
    wl = tuple(float(w) for w in wavelengths)
    if len(wl) != field.shape[1]:
        raise ValueError(f"{who}: {len(wl)} wavelengths for a field of {field.shape[1]} channels")
    cfg = tolerance_cfg(fab, who)
    if idx is not None:
        if not torch.is_tensor(idx) or idx.shape != height.shape or idx.device != height.device:
            raise ValueError(f"{who}: idx must be an integer tensor of the map's shape on its device")
        idx = idx.to(torch.int32).contiguous()
    elif any(v != 0.0 for v in cfg[1]):
        raise ValueError(f"{who}: a per-level error needs idx, the level index of every map pixel")
    state, stream = noise_state(field, rng)
    out, heights = _ToleranceModulate.apply(field, height, idx, state, (K, first, stream, float(eps), float(tand), wl,
                                                                        cfg, bool(return_heights)))
    return (out, heights) if return_heights else out
