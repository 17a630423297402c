"""Device entry points for the propagators: thin torch glue over the C-ABI.

Each function takes CUDA(HIP) complex64 tensors plus HOST scalars (wavelengths,
spacing, z) and enqueues the hand-written gfx950 kernels of libthzdoe.so on the
current torch stream.  The autograd Functions route backward through the same
kernels (the ASM adjoint == ASM with conj(H)).  There is no CPU
path: a CPU tensor is an error.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import threading
import typing

import torch

from . import _lib
from ._call import _launch, _require_device, call, loss_stats


def kernel_dtype(data: torch.Tensor, who: str, wavelengths=None) -> torch.Tensor:
    """The field in the precision the reference computes it in (DataType/ElectricField.py:85-90):
    complex128 when the data is complex128 / float64 or the wavelength tensor is float64 (torch's
    promotion; the reference's test_czt.py:12 runs that way), else complex64.  The complex128
    fields run the fp64 kernels (csrc/thz_f64.hip), the rest the fp32 ones; real data is promoted
    as torch's complex products promote it."""
    fp64 = data.dtype in (torch.complex128, torch.float64) or (
        torch.is_tensor(wavelengths) and wavelengths.dtype == torch.float64)
    if data.dtype not in (torch.complex64, torch.complex128, torch.float32, torch.float64, torch.float16,
                          torch.bfloat16):
        raise TypeError(f"{who}: the MI355X kernels compute in complex64 or complex128; got {data.dtype}")
    want = torch.complex128 if fp64 else torch.complex64
    return data if data.dtype == want else data.to(want)


def _bandlimit(b):
    """thz_asm_desc.bandlimit: the code itself, or the code of a name (_lib.BANDLIMIT)."""
    return b if isinstance(b, int) else _lib.BANDLIMIT[b]


def asm_padding(H, W, padding_scale, do_padding=True):
    """pad = floor(s N / 2), P = N + 2 pad (Props/ASM_Prop.py:119-136)."""
    if not do_padding:
        return 0, 0
    sh, sw = padding_scale
    return int(math.floor(float(sh) * H / 2)), int(math.floor(float(sw) * W / 2))


def _asm_desc(B, C, H, W, pad_h, pad_w, unpad, bandlimit, wavelengths, spacing, zs, adjoint, z_chunk=0,
              mask=None, z_dev=None):
    """thz_asm_desc; ``mask``: an ApertureDesc on the output grid (thz_asm_desc.window_mask);
    ``z_dev``: a float32 device tensor [Z] the kernels read the plane distances from
    (thz_asm_desc.z_dev: graph-replayable planes; ``zs`` then only gives their count)."""
    if z_dev is not None and (z_dev.dtype != torch.float32 or not z_dev.is_contiguous() or z_dev.numel() != len(zs)
                              or z_dev.device.type != "cuda"):
        raise ValueError(f"z_dev: a contiguous float32 device tensor of {len(zs)} planes")
    wl = _lib.float_array(wavelengths)
    zv = _lib.float_array(zs)
    d = _lib.AsmDesc(B=B, C=C, H=H, W=W, pad_h=pad_h, pad_w=pad_w, unpad=int(bool(unpad)),
                     bandlimit=int(bandlimit), Z=len(zs), adjoint=int(adjoint), z_chunk=int(z_chunk),
                     dx=float(spacing[0]), dy=float(spacing[1]),
                     wavelengths=ctypes.cast(wl, ctypes.POINTER(ctypes.c_float)),
                     z=ctypes.cast(zv, ctypes.POINTER(ctypes.c_float)),
                     window_mask=ctypes.addressof(mask) if mask is not None else None,
                     z_dev=z_dev.data_ptr() if z_dev is not None else None)
    d._keep = (wl, zv, mask, z_dev)
    return d


def window_mask_fusable(H, W, pad_h, pad_w, unpad, Z=1):
    """True when the library folds an aperture into the propagation (thz_asm_desc.window_mask): the
    300-point layer geometry of the cfg4 / cfg5 systems (100-pixel fields, padding 2, cropped)."""
    return H == W == 100 and pad_h == pad_w == 100 and bool(unpad) and Z == 1


def asm_apply(data, wavelengths, spacing, zs, pad_h, pad_w, unpad, bandlimit, adjoint=False, z_chunk=0,
              out=None, mask=None, z_dev=None):
    """Raw launch: forward data [B,C,H,W] -> [Z,B,C,Ho,Wo]; adjoint [Z,B,C,Ho,Wo] -> [B,C,H,W], the sum
    over the Z planes of each plane's adjoint (one pipeline: the column pass sums the planes'
    spectra, thz_asm_forward with adjoint = 1)."""
    _require_device(data, "ASM")
    if mask is not None:
        # the folded aperture exists in the complex64 300-point row passes only, and its adjoint takes
        # one plane: refuse here, in the forward, rather than drop the mask or fail in backward
        if data.dtype != torch.complex64:
            raise TypeError(f"ASM window mask: complex64 fields only, got {data.dtype} (apply the aperture "
                            "separately)")
        if len(zs) != 1:
            raise ValueError(f"ASM window mask: one z-plane per call, got {len(zs)}")
    if data.dtype == torch.complex128:
        if z_dev is not None:
            raise TypeError("ASM z_dev: complex64 fields only (the fp64 kernels take host planes)")
        return _asm64_apply(data, wavelengths, spacing, zs, pad_h, pad_w, unpad, bandlimit, adjoint, out)
    if data.dtype != torch.complex64:
        raise TypeError(f"ASM kernels compute in complex64 or complex128; got {data.dtype}")
    L = _lib.lib()
    data = data.contiguous()
    (B, C, H, W), out_shape = _asm_shapes(data, zs, pad_h, pad_w, unpad, adjoint)
    d = _asm_desc(B, C, H, W, pad_h, pad_w, unpad, bandlimit, wavelengths, spacing, zs, adjoint, z_chunk, mask, z_dev)
    if out is None:
        out = torch.empty(out_shape, dtype=torch.complex64, device=data.device)
    _launch(L.thz_asm_workspace_size, L.thz_asm_forward, d, data.device, data, out)
    return out


def _asm_shapes(data, zs, pad_h, pad_w, unpad, adjoint):
    """(field shape (B, C, H, W), output shape) of an ASM launch on ``data``: the field itself
    forward, the [Z,B,C,Ho,Wo] cotangent of its planes in the adjoint."""
    if adjoint:
        Z, B, C, Ho, Wo = data.shape
        if Z != len(zs):
            raise ValueError(f"adjoint: {Z} gradient planes for {len(zs)} z values")
        field = (B, C, Ho - (0 if unpad else 2 * pad_h), Wo - (0 if unpad else 2 * pad_w))
        return field, field
    B, C, H, W = data.shape
    Ho, Wo = (H, W) if unpad else (H + 2 * pad_h, W + 2 * pad_w)
    return (B, C, H, W), (len(zs), B, C, Ho, Wo)


ASM_SLICE_HEIGHTS = (1024, 2048, 4096, 8192, 16384)  # padded heights thz_asm_slice_forward serves


def asm_slice_native(padded_height):
    """True when the z-x slice kernels serve this padded height (the compile-time power-of-two
    column passes); other heights slice the full planes (ASM_prop.propagate_zx)."""
    return int(padded_height) in ASM_SLICE_HEIGHTS


def _asm64_apply(data, wavelengths, spacing, zs, pad_h, pad_w, unpad, bandlimit, adjoint=False, out=None):
    """complex128 ASM (thz_asm64_forward): the same shapes as asm_apply; the fp64 adjoint runs one
    launch per plane and sums them."""
    data = data.contiguous()
    field, out_shape = _asm_shapes(data, zs, pad_h, pad_w, unpad, adjoint)
    if adjoint:
        res = None
        for k, z in enumerate(zs):
            gk = _asm64_launch(data[k:k + 1], field, wavelengths, spacing, [z], pad_h, pad_w, unpad, bandlimit,
                               True, torch.empty(field, dtype=torch.complex128, device=data.device))
            res = gk if res is None else res + gk
        return res
    if out is None:
        out = torch.empty(out_shape, dtype=torch.complex128, device=data.device)
    return _asm64_launch(data, field, wavelengths, spacing, zs, pad_h, pad_w, unpad, bandlimit, False, out)


def _asm64_launch(data, shape, wavelengths, spacing, zs, pad_h, pad_w, unpad, bandlimit, adjoint, out):
    L = _lib.lib()
    B, C, H, W = shape
    wl = _lib.double_array(wavelengths)
    zv = _lib.double_array(zs)
    d = _lib.AsmDesc64(B=B, C=C, H=H, W=W, pad_h=pad_h, pad_w=pad_w, unpad=int(bool(unpad)), bandlimit=int(bandlimit),
                       Z=len(zs), adjoint=int(adjoint), dx=float(spacing[0]), dy=float(spacing[1]),
                       wavelengths=ctypes.cast(wl, ctypes.POINTER(ctypes.c_double)),
                       z=ctypes.cast(zv, ctypes.POINTER(ctypes.c_double)))
    _launch(L.thz_asm64_workspace_size, L.thz_asm64_forward, d, data.device, data, out)
    return out


def asm_plan_info(B, C, H, W, pad_h, pad_w, unpad, bandlimit, wavelengths, spacing, zs, z_chunk=0):
    """(kept spectral columns, z-planes per column pass) of the library's plan."""
    d = _asm_desc(B, C, H, W, pad_h, pad_w, unpad, bandlimit, wavelengths, spacing, zs, False, z_chunk)
    n, zc = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.lib().thz_asm_band(ctypes.byref(d), ctypes.byref(n), ctypes.byref(zc)))
    return n.value, zc.value


def asm_band_columns(B, C, H, W, pad_h, pad_w, unpad, bandlimit, wavelengths, spacing, zs):
    return asm_plan_info(B, C, H, W, pad_h, pad_w, unpad, bandlimit, wavelengths, spacing, zs)[0]


class _AsmFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, data, wavelengths, spacing, zs, pad_h, pad_w, unpad, bandlimit, z_chunk, mask, z_dev):
        ctx.cfg = (wavelengths, spacing, zs, pad_h, pad_w, unpad, bandlimit, mask, z_dev)
        return asm_apply(data, wavelengths, spacing, zs, pad_h, pad_w, unpad, bandlimit, False, z_chunk, mask=mask,
                         z_dev=z_dev)

    @staticmethod
    def backward(ctx, g):
        wavelengths, spacing, zs, pad_h, pad_w, unpad, bandlimit, mask, z_dev = ctx.cfg
        # one adjoint launch for all planes: sum_z A_z^H g_z, the sum taken in the column pass (the
        # window mask, when folded, on the adjoint's input)
        gin = asm_apply(g.contiguous(), wavelengths, spacing, zs, pad_h, pad_w, unpad, bandlimit, True, mask=mask,
                        z_dev=z_dev)
        return gin, None, None, None, None, None, None, None, None, None, None


def asm_transfer_function(wavelengths, spacing, z, H, W, pad_h, pad_w, bandlimit, device):
    """ASM_prop.create_kernel's table (Props/ASM_Prop.py:212-311): [1, C, Ph, Pw] complex64 on the
    centred frequency grid, computed by the HIP kernel the propagators evaluate on the fly."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"ASM transfer function: the MI355X path needs a ROCm device (got {dev}); "
                           "this framework has no CPU compute path")
    bl = _bandlimit(bandlimit)
    d = _asm_desc(1, len(wavelengths), int(H), int(W), int(pad_h), int(pad_w), True, bl, wavelengths, spacing,
                  [float(z)], False)
    out = torch.empty((1, len(wavelengths), H + 2 * pad_h, W + 2 * pad_w), dtype=torch.complex64, device=dev)
    call(_lib.lib().thz_asm_transfer_function, d, out, device=dev)
    return out


def rs_kernel(meshx, meshy, z, wavelengths):
    """exp(ikr) z/(2 pi r^2) (1/r - ik) on the meshes for each wavelength (Props/CZT_Prop.py:44-57,
    Props/RSC_Prop.py:157-160): [1, C, *mesh.shape] complex64 from the HIP kernel thz_rs_kernel."""
    _require_device(meshx, "RS kernel")
    mx, my = torch.broadcast_tensors(meshx, meshy)
    shape = tuple(mx.shape)
    mx = mx.detach().to(torch.float32).contiguous().reshape(-1)
    my = my.detach().to(device=mx.device, dtype=torch.float32).contiguous().reshape(-1)
    wl = [float(v) for v in wavelengths]
    arr = _lib.float_array(wl)
    out = torch.empty((1, len(wl)) + shape, dtype=torch.complex64, device=mx.device)
    call(_lib.lib().thz_rs_kernel, mx, my, int(mx.numel()), ctypes.c_float(float(z)), ctypes.cast(arr, ctypes.c_void_p),
         len(wl), out, device=mx.device)
    return out


def asm_propagate(data, wavelengths, spacing, zs, pad_h, pad_w, unpad=True, bandlimit="exact", z_chunk=0,
                  mask=None, z_dev=None):
    """Differentiable ASM over Z planes: [B,C,H,W] -> [Z,B,C,Ho,Wo] (HIP kernels); ``mask``: an
    aperture folded onto the output (window_mask_fusable geometry only); ``z_dev``: the planes in
    device memory (_asm_desc)."""
    bl = _bandlimit(bandlimit)
    return _AsmFunction.apply(data, list(map(float, wavelengths)), tuple(map(float, spacing)),
                              list(map(float, zs)), int(pad_h), int(pad_w), bool(unpad), bl, int(z_chunk), mask, z_dev)


class _AsmModulatedFunction(torch.autograd.Function):
    """ASM forward of DOELayer.modulate(field) in one pipeline (thz_asm_forward_modulated): the row
    pass applies t_c(h + noise) in its loader.  Backward: the ASM adjoint summed over the planes
    (one launch), then the modulate backward kernel (grad_field, grad_height) -- or, when the height
    map comes straight from a quantizer of the field's size (doe.QuantLink), the modulate and
    quantizer backward in one kernel (grad_field, grad_weight)."""

    @staticmethod
    def forward(ctx, field, height, weight, pend, wavelengths, spacing, zs, pad_h, pad_w, unpad, bandlimit, mask,
                z_dev):
        _require_device(field, "ASM")
        field = field.contiguous()
        h = height.detach().contiguous().float()
        B, C, H, W = field.shape
        Ho, Wo = (H, W) if unpad else (H + 2 * pad_h, W + 2 * pad_w)
        d = _asm_desc(B, C, H, W, pad_h, pad_w, unpad, bandlimit, wavelengths, spacing, zs, False, mask=mask,
                      z_dev=z_dev)
        m = pend.desc()
        L = _lib.lib()
        out = torch.empty((len(zs), B, C, Ho, Wo), dtype=torch.complex64, device=field.device)
        hfull = torch.empty((H, W), dtype=torch.float32, device=field.device)
        _launch(L.thz_asm_workspace_size, L.thz_asm_forward_modulated, d, field.device, m, field, h, pend.noise, hfull,
                out)
        if pend.hfull is None:
            pend.hfull = hfull
        ctx.save_for_backward(field, h)
        ctx.pend = pend
        ctx.cfg = (wavelengths, spacing, zs, pad_h, pad_w, unpad, bandlimit, mask, z_dev)
        return out

    @staticmethod
    def backward(ctx, g):
        field, h = ctx.saved_tensors
        pend = ctx.pend
        wavelengths, spacing, zs, pad_h, pad_w, unpad, bandlimit, mask, z_dev = ctx.cfg
        gm = asm_apply(g.contiguous(), wavelengths, spacing, zs, pad_h, pad_w, unpad, bandlimit, True, mask=mask,
                       z_dev=z_dev)
        gf, gh, gw = _doe_backward(ctx, gm, field, h, pend)
        return (gf, gh, gw) + (None,) * 11


def _doe_inputs(pend):
    """(height, weight) inputs of a fused function for the pending modulation ``pend``: with a
    fusable quantizer link (doe.QuantLink) the weight is differentiated directly, in one kernel with
    the modulate backward (_doe_backward), and the height map enters detached."""
    if pend.quant is None:
        return pend.height, None
    return pend.height.detach(), pend.quant.weight


def _doe_backward(ctx, gm, field, h, pend):
    """(grad_field, grad_height, grad_weight) of the modulation behind a fused function, whose
    inputs 0, 1, 2 are (field, height, weight): one thz_doe_quant_backward when the quantizer is
    linked, else thz_doe_modulate_backward."""
    from . import doe as _doe
    if pend.quant is not None and ctx.needs_input_grad[2]:
        gf, gw = _doe.modulate_quant_backward(gm, field, h, pend.noise, pend.tol, pend.eps, pend.tand,
                                              pend.wavelengths, pend.quant, ctx.needs_input_grad[0], rng=pend.rng)
        return gf, None, gw
    gf, gh = _doe.modulate_backward(gm, field, h, pend.noise, pend.tol, pend.eps, pend.tand, pend.wavelengths,
                                    ctx.needs_input_grad[0], ctx.needs_input_grad[1], rng=pend.rng)
    return gf, gh, None


def asm_propagate_modulated(pend, wavelengths, spacing, zs, pad_h, pad_w, unpad=True, bandlimit="exact", mask=None,
                            z_dev=None):
    """Differentiable fused DOE modulation + ASM over Z planes: [B,C,H,W] -> [Z,B,C,Ho,Wo]; ``mask``
    and ``z_dev`` as asm_propagate."""
    bl = _bandlimit(bandlimit)
    height, weight = _doe_inputs(pend)
    return _AsmModulatedFunction.apply(pend.field, height, weight, pend, list(map(float, wavelengths)),
                                       tuple(map(float, spacing)), list(map(float, zs)), int(pad_h), int(pad_w),
                                       bool(unpad), bl, mask, z_dev)


class _AsmLossFunction(torch.autograd.Function):
    """Z z-planes of ASM (optionally of a pending DOE modulation) whose row-inverse pass also
    accumulates the QAT loss mean((normalize(|E|^2) - target)^2) (thz_asm_forward_loss) -- for
    Z > 1 the sum over the planes of each plane's mean, the multi-plane notebooks' summed MSEs,
    the target [tB, tC, Ho, Wo] broadcast over the Z B plane-major items (tB in {1, Z B}).
    Outputs (out [Z,B,C,Ho,Wo], loss []).  Backward: the ASM adjoint (summed over the planes) of the
    loss gradient of the stored field, formed in the adjoint's row pass (thz_asm_adjoint_loss;
    plus the out cotangent when out is used elsewhere), then the DOE layer's backward when a
    modulation was fused."""

    @staticmethod
    def forward(ctx, field, height, weight, target, pend, wavelengths, spacing, zs, pad_h, pad_w, unpad, bandlimit,
                z_dev=None):
        ctx.set_materialize_grads(False)
        if field.dtype != torch.complex64:  # thz_asm_forward_loss reads float2 pairs
            raise TypeError(f"fused ASM loss computes in complex64 fields; got {field.dtype}")
        _require_device(field, "ASM")
        field = field.contiguous()
        B, C, H, W = field.shape
        Ho, Wo = (H, W) if unpad else (H + 2 * pad_h, W + 2 * pad_w)
        Z = len(zs)
        t4 = target.detach().float().contiguous()
        t4 = t4.reshape((1,) * (4 - t4.dim()) + tuple(t4.shape))
        if tuple(t4.shape[-2:]) != (Ho, Wo) or t4.shape[0] not in (1, Z * B) or t4.shape[1] not in (1, C):
            raise ValueError(f"target {tuple(target.shape)} does not broadcast to field {(Z * B, C, Ho, Wo)}")
        d = _asm_desc(B, C, H, W, pad_h, pad_w, unpad, bandlimit, wavelengths, spacing, zs, False, z_dev=z_dev)
        ld = _lib.LossDesc(B=Z * B, C=C, H=Ho, W=Wo, tB=t4.shape[0], tC=t4.shape[1])
        L = _lib.lib()
        dev = field.device
        out = torch.empty((Z, B, C, Ho, Wo), dtype=torch.complex64, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        stats = loss_stats(ld, dev)
        h = hfull = noise = None
        m = None
        if pend is not None:
            h = height.detach().contiguous().float()
            hfull = torch.empty((H, W), dtype=torch.float32, device=dev)
            noise = pend.noise
            m = pend.desc()
        _launch(L.thz_asm_workspace_size, L.thz_asm_forward_loss, d, dev, m, field, h, noise, hfull, ld, t4, out, loss,
                stats)
        if pend is not None and pend.hfull is None:
            pend.hfull = hfull
        ctx.save_for_backward(field, h, out, t4, stats)
        ctx.pend = pend
        ctx.cfg = (wavelengths, spacing, zs, pad_h, pad_w, unpad, bandlimit, z_dev)
        ctx.ldesc = (B, C, Ho, Wo, t4.shape[0], t4.shape[1])
        return out, loss

    @staticmethod
    def backward(ctx, g_out, g_loss):
        field, h, out, t4, stats = ctx.saved_tensors
        wavelengths, spacing, zs, pad_h, pad_w, unpad, bandlimit, z_dev = ctx.cfg
        if g_loss is None and g_out is None:
            return (None,) * 13
        if g_loss is None:
            gm = asm_apply(g_out.contiguous(), wavelengths, spacing, zs, pad_h, pad_w, unpad, bandlimit, True,
                           z_dev=z_dev)
        else:
            # the loss gradient is formed in the adjoint's row pass (thz_asm_adjoint_loss)
            B, C, Ho, Wo, tB, tC = ctx.ldesc
            H, W = field.shape[-2:]
            ld = _lib.LossDesc(B=len(zs) * B, C=C, H=Ho, W=Wo, tB=tB, tC=tC)
            d = _asm_desc(B, C, H, W, pad_h, pad_w, unpad, bandlimit, wavelengths, spacing, zs, True, z_dev=z_dev)
            L = _lib.lib()
            gm = torch.empty((B, C, H, W), dtype=torch.complex64, device=out.device)
            g = g_loss.detach().float().contiguous()
            go = g_out.contiguous() if g_out is not None else None
            _launch(L.thz_asm_workspace_size, L.thz_asm_adjoint_loss, d, out.device, ld, out, t4, stats, g, go, gm)
        gh = gw = None
        pend = ctx.pend
        if pend is None:
            gf = gm
        else:
            gf, gh, gw = _doe_backward(ctx, gm, field, h, pend)
        return (gf, gh, gw) + (None,) * 10


def asm_propagate_loss(x, target, wavelengths, spacing, z, pad_h, pad_w, unpad=True, bandlimit="exact", pend=None,
                       z_dev=None):
    """Differentiable ASM fused with the QAT loss: (out [Z,B,C,Ho,Wo], loss []).  ``z``: one
    distance, or a list of Z planes (the loss is then the sum of the planes' means, the target
    broadcast over the Z B plane-major items); ``z_dev`` as asm_propagate.  ``pend``
    (doe.PendingModulation, not yet formed): propagate its modulation of ``pend.field`` (``x`` is
    then ignored), as asm_propagate_modulated."""
    bl = _bandlimit(bandlimit)
    zs = [float(v) for v in z] if isinstance(z, (list, tuple)) else [float(z)]
    if len(zs) > _lib.THZ_MAX_Z:
        raise ValueError(f"the fused loss takes at most {_lib.THZ_MAX_Z} planes per call")
    field, (height, weight) = (pend.field, _doe_inputs(pend)) if pend is not None else (x, (None, None))
    return _AsmLossFunction.apply(field, height, weight, target, pend, list(map(float, wavelengths)),
                                  tuple(map(float, spacing)), zs, int(pad_h), int(pad_w), bool(unpad), bl, z_dev)


class _Deferral(threading.local):
    active = False


_DEFER = _Deferral()


@contextlib.contextmanager
def deferred_output():
    """Inside this block ASM_prop.forward returns its output field unevaluated: the propagation
    runs when the field's ``data`` is first read -- or, when the first reader is the QAT loss
    (optics.field_intensity_mse), as one pipeline with the loss folded into its last pass
    (thz_asm_forward_loss).  The trainers wrap their forward in it; the deferred propagation reads
    its input field when it runs, so the input must not be modified in between."""
    prev = _DEFER.active
    _DEFER.active = True
    try:
        yield
    finally:
        _DEFER.active = prev


def deferring():
    return _DEFER.active


def fft_rows(x, inverse=False):
    """Unnormalised batched 1-D FFT along the last axis with the LDS Stockham kernel (complex128
    input: the fp64 transform)."""
    _require_device(x, "fft_rows")
    x = x.contiguous()
    x = x if x.dtype == torch.complex128 else x.to(torch.complex64)
    out = torch.empty_like(x)
    n = x.shape[-1]
    rows = x.numel() // n
    fn = _lib.lib().thz_fft64_rows if x.dtype == torch.complex128 else _lib.lib().thz_fft_rows
    call(fn, x, out, rows, n, int(inverse), device=x.device)
    return out


def _by_dtype(tag, dtype):
    """(descriptor class, host array maker, ctypes scalar, size_fn, run_fn) of the propagator ``tag``
    ("czt" / "rsc") in the field's precision: the fp64 entries for complex128, else the fp32 ones."""
    L = _lib.lib()
    if dtype == torch.complex128:
        return (getattr(_lib, f"{tag.capitalize()}Desc64"), _lib.double_array, ctypes.c_double,
                getattr(L, f"thz_{tag}64_workspace_size"), getattr(L, f"thz_{tag}64_forward"))
    return (getattr(_lib, f"{tag.capitalize()}Desc"), _lib.float_array, ctypes.c_float,
            getattr(L, f"thz_{tag}_workspace_size"), getattr(L, f"thz_{tag}_forward"))


def czt_apply(data, wavelengths, spacing, z, outH, outW, odx, ody, adjoint=False, field_hw=None):
    """Chirp-z propagation [B,C,H,W] -> [B,C,outW,outH] (Props/CZT_Prop.py:252-314) on the HIP kernels.

    adjoint: the autograd backward, [B,C,outW,outH] -> [B,C,H,W] with (H, W) = field_hw."""
    _require_device(data, "CZT")
    if data.dtype not in (torch.complex64, torch.complex128):
        raise TypeError(f"CZT kernels compute in complex64 or complex128; got {data.dtype}")
    data = data.contiguous()
    B, C = data.shape[:2]
    H, W = (int(v) for v in (field_hw if adjoint else data.shape[-2:]))
    if adjoint and tuple(data.shape[-2:]) != (int(outW), int(outH)):
        raise ValueError(f"CZT adjoint: gradient {tuple(data.shape)} is not [B, C, outW, outH]")
    desc, array, ctype, size_fn, run_fn = _by_dtype("czt", data.dtype)
    wl = array(wavelengths)
    d = desc(B=B, C=C, H=H, W=W, outH=int(outH), outW=int(outW), dx=float(spacing[0]), dy=float(spacing[1]),
             odx=float(odx), ody=float(ody), z=float(z), wavelengths=ctypes.cast(wl, ctypes.POINTER(ctype)),
             adjoint=int(bool(adjoint)))
    oshape = (B, C, H, W) if adjoint else (B, C, int(outW), int(outH))
    out = torch.empty(oshape, dtype=data.dtype, device=data.device)
    _launch(size_fn, run_fn, d, data.device, data, out)
    return out


def _czt_slice_desc(B, C, H, W, outH, outW, spacing, odx, ody, wavelengths, zs, row):
    """thz_czt_slice_desc (the host arrays are kept alive by the descriptor)."""
    wl = _lib.float_array(wavelengths)
    zv = _lib.float_array(zs)
    d = _lib.CztSliceDesc(B=int(B), C=int(C), H=int(H), W=int(W), outH=int(outH), outW=int(outW),
                          dx=float(spacing[0]), dy=float(spacing[1]), odx=float(odx), ody=float(ody), Z=len(zs),
                          z=ctypes.cast(zv, ctypes.POINTER(ctypes.c_float)),
                          wavelengths=ctypes.cast(wl, ctypes.POINTER(ctypes.c_float)), row=int(row))
    d._keep = (wl, zv)
    return d


def rsc_apply(data, wavelengths, spacing, z, vectorial=False, adjoint=False, field_hw=None):
    """Rayleigh-Sommerfeld convolution (Props/RSC_Prop.py:170-321) on the HIP kernels.

    [B,C,H,W] -> [Bo,C,Ph-H,Pw-W], Ph = H + 2 floor(H/2); vectorial: Ex/Ey planes in, 3 planes out.
    adjoint: the autograd backward of the scalar convolution, [B,C,Ph-H,Pw-W] -> [B,C,H,W] with
    (H, W) = field_hw, the forward field's shape.
    """
    _require_device(data, "RSC")
    if data.dtype not in (torch.complex64, torch.complex128):
        raise TypeError(f"RSC kernels compute in complex64 or complex128; got {data.dtype}")
    data = data.contiguous()
    B, C = data.shape[:2]
    H, W = field_hw if adjoint else data.shape[-2:]
    desc, array, ctype, size_fn, run_fn = _by_dtype("rsc", data.dtype)
    wl = array(wavelengths)
    d = desc(B=B, C=C, H=int(H), W=int(W), vectorial=int(bool(vectorial)), dx=float(spacing[0]), dy=float(spacing[1]),
             z=float(z), wavelengths=ctypes.cast(wl, ctypes.POINTER(ctype)), adjoint=int(bool(adjoint)))
    if adjoint:
        if tuple(data.shape[-2:]) != (2 * (H // 2), 2 * (W // 2)):
            raise ValueError(f"RSC adjoint: gradient {tuple(data.shape)} does not match field {(H, W)}")
        out = torch.empty((B, C, int(H), int(W)), dtype=data.dtype, device=data.device)
    else:
        Bo = 3 if vectorial else B
        out = torch.empty((Bo, C, 2 * (H // 2), 2 * (W // 2)), dtype=data.dtype, device=data.device)
    if out.numel() == 0 or data.numel() == 0:
        # H or W = 1: the reference's [..., H:, W:] window is empty (Props/RSC_Prop.py:203-207; run
        # here: [B, C, 0, 2 (W // 2)] and the like); the adjoint of an empty output is zero
        return out.zero_()
    _launch(size_fn, run_fn, d, data.device, data, out)
    return out


def _rsc_slice_desc(B, C, H, W, vectorial, spacing, wavelengths, zs, row):
    """thz_rsc_slice_desc (the host arrays are kept alive by the descriptor)."""
    wl = _lib.float_array(wavelengths)
    zv = _lib.float_array(zs)
    d = _lib.RscSliceDesc(B=int(B), C=int(C), H=int(H), W=int(W), vectorial=int(bool(vectorial)),
                          dx=float(spacing[0]), dy=float(spacing[1]), Z=len(zs),
                          z=ctypes.cast(zv, ctypes.POINTER(ctypes.c_float)),
                          wavelengths=ctypes.cast(wl, ctypes.POINTER(ctypes.c_float)), row=int(row))
    d._keep = (wl, zv)
    return d


# -- z-x slices: one output row of every plane of a z-sweep -------------------------------------
# The ASM, CZT and RSC / VRS slice kernels differ; the glue above them does not.  A family says what
# differs (_SliceFamily), and the launches, the autograd Function and the THZ_MAX_Z driver below
# exist once.  ``geo`` is the family's geometry tuple, the trailing positional arguments of its
# ``*_slice_apply``: ASM (pad_h, pad_w, unpad, bandlimit), CZT (outH, outW, odx, ody), RSC (vectorial,).

class _SliceFamily(typing.NamedTuple):
    label: str                # "ASM": the prefix of the error texts
    entries: tuple            # library entry names: forward, its workspace size, adjoint, its workspace size
    row_positional: bool      # the row is an argument of the entry points (ASM), else a descriptor field
    desc: typing.Callable     # (field shape, geo, wavelengths, spacing, zs, row, adjoint) -> descriptor
    out_shape: typing.Callable    # (Z, field shape, geo) -> the forward's output shape
    field_shape: typing.Callable  # (cotangent, zs, geo, extra) -> (B, C, H, W), or ValueError
    apply: typing.Callable    # the public raw forward (data, wavelengths, spacing, zs, row, geo, out=None)
    adjoint: typing.Callable  # the public raw adjoint (g, wavelengths, spacing, zs, row, geo, field shape)
    empty_window: bool = False    # an empty output is returned (adjoint: zero) without a launch


def _slice_entries(tag):
    return (f"thz_{tag}_slice_forward", f"thz_{tag}_slice_workspace_size",
            f"thz_{tag}_slice_adjoint", f"thz_{tag}_slice_adjoint_workspace_size")


def _asm_slice_field(g, zs, geo, height):
    Z, B, C, Wo = g.shape
    if Z != len(zs):
        raise ValueError(f"ASM slice adjoint: {Z} gradient rows for {len(zs)} z values")
    return B, C, int(height), Wo - (0 if geo[2] else 2 * geo[1])


def _czt_slice_field(g, zs, geo, field_hw):
    Z, B, C, n = g.shape
    if Z != len(zs) or n != int(geo[0]):
        raise ValueError(f"CZT slice adjoint: gradient {tuple(g.shape)} is not [{len(zs)}, B, C, {int(geo[0])}]")
    H, W = (int(v) for v in field_hw)
    return B, C, H, W


def _rsc_slice_out(Z, shape, geo):
    B, C, _, W = shape
    return Z, 3 if geo[0] else B, C, 2 * (W // 2)


def _rsc_slice_field(g, zs, geo, field_shape):
    shape = tuple(int(v) for v in field_shape)
    gshape = _rsc_slice_out(len(zs), shape, geo)
    if tuple(g.shape) != gshape:
        raise ValueError(f"RSC slice adjoint: gradient {tuple(g.shape)} is not {list(gshape)}")
    return shape


# ``apply`` / ``adjoint`` name the public functions in lambdas, so they are looked up in this module
# when called: what serves a propagate_zx is what a caller of the public function would get.
# A fourth slice is one more entry here and its three public wrappers below.
_SLICE_FAMILIES = {
    "asm": _SliceFamily(
        "ASM", _slice_entries("asm"), True,
        desc=lambda s, geo, wl, sp, zs, row, adj: _asm_desc(*s, *geo, wl, sp, zs, adj),
        out_shape=lambda Z, s, geo: (Z, s[0], s[1], s[3] if geo[2] else s[3] + 2 * geo[1]),
        field_shape=_asm_slice_field,
        apply=lambda x, wl, sp, zs, row, geo, out=None: asm_slice_apply(x, wl, sp, zs, row, *geo, out=out),
        adjoint=lambda g, wl, sp, zs, row, geo, s: asm_slice_adjoint(g, wl, sp, zs, row, *geo, s[2])),
    "czt": _SliceFamily(
        "CZT", _slice_entries("czt"), False,
        desc=lambda s, geo, wl, sp, zs, row, adj: _czt_slice_desc(*s, geo[0], geo[1], sp, geo[2], geo[3], wl, zs, row),
        out_shape=lambda Z, s, geo: (Z, s[0], s[1], int(geo[0])),
        field_shape=_czt_slice_field,
        apply=lambda x, wl, sp, zs, row, geo, out=None: czt_slice_apply(x, wl, sp, zs, row, *geo, out=out),
        adjoint=lambda g, wl, sp, zs, row, geo, s: czt_slice_adjoint(g, wl, sp, zs, row, *geo, s[2:])),
    "rsc": _SliceFamily(
        "RSC", _slice_entries("rsc"), False,
        desc=lambda s, geo, wl, sp, zs, row, adj: _rsc_slice_desc(*s, geo[0], sp, wl, zs, row),
        out_shape=_rsc_slice_out,
        field_shape=_rsc_slice_field,
        apply=lambda x, wl, sp, zs, row, geo, out=None: rsc_slice_apply(x, wl, sp, zs, row, *geo, out=out),
        adjoint=lambda g, wl, sp, zs, row, geo, s: rsc_slice_adjoint(g, wl, sp, zs, row, s, *geo),
        empty_window=True),  # W = 1: the reference's [..., W:] window is empty
}


def _slice_launch(fam, adjoint, src, wavelengths, spacing, zs, row, geo, extra, out):
    """The one raw launch of a slice family: forward src = the field [B,C,H,W] -> ``out_shape``;
    adjoint src = the cotangent of that -> [B,C,H,W], the field shape recovered with ``extra``.
    At most THZ_MAX_Z planes; ``out``, when given, is checked and every element of it overwritten."""
    who = f"{fam.label} slice adjoint" if adjoint else f"{fam.label} slice"
    _require_device(src, who)
    if src.dtype != torch.complex64:
        raise TypeError(f"{fam.label} slice kernels compute in complex64; got {src.dtype}")
    L = _lib.lib()
    src = src.contiguous()
    field = fam.field_shape(src, zs, geo, extra) if adjoint else tuple(src.shape)
    d = fam.desc(field, geo, wavelengths, spacing, zs, row, adjoint)
    shape = tuple(field) if adjoint else tuple(fam.out_shape(len(zs), field, geo))
    if out is None:
        out = torch.empty(shape, dtype=torch.complex64, device=src.device)
    elif tuple(out.shape) != shape or out.dtype != torch.complex64 or not out.is_contiguous():
        raise ValueError(f"{who}: out must be a contiguous complex64 {shape} tensor")
    if fam.empty_window and (src if adjoint else out).numel() == 0:
        return out.zero_() if adjoint else out
    run, size = (getattr(L, name) for name in fam.entries[2 * adjoint:2 * adjoint + 2])
    _launch(size, run, d, src.device, *((int(row),) if fam.row_positional else ()), src, out)
    return out


class _SliceFunction(torch.autograd.Function):
    """A z-x slice with its native backward: forward the family's ``*_slice_apply``, backward its
    ``*_slice_adjoint``.  A linear map: nothing is saved but the family and the configuration."""

    @staticmethod
    def forward(ctx, data, fam, wavelengths, spacing, zs, row, geo):
        ctx.cfg = (fam, wavelengths, spacing, zs, row, geo, tuple(data.shape))
        return fam.apply(data, wavelengths, spacing, zs, row, geo)

    @staticmethod
    def backward(ctx, g):
        fam, *cfg = ctx.cfg
        return (fam.adjoint(g, *cfg),) + (None,) * 6


def _slice_sweep(fam, data, wavelengths, spacing, zs, row, geo, diff):
    """A z-sweep of any length on the slice kernels of ``fam``, in chunks of THZ_MAX_Z planes.
    ``diff``: each chunk through _SliceFunction (backward: the family's adjoint), concatenated when
    there is more than one; else the whole [Z, ...] result is allocated once and each chunk written
    into its part of it (no copy, no second allocation; ``data`` enters detached)."""
    wl, sp, zs = list(map(float, wavelengths)), tuple(map(float, spacing)), list(map(float, zs))
    max_z = _lib.THZ_MAX_Z
    if diff:
        outs = [_SliceFunction.apply(data, fam, wl, sp, zs[k:k + max_z], row, geo) for k in range(0, len(zs), max_z)]
        return outs[0] if len(outs) == 1 else torch.cat(outs, 0)
    data = data.detach().contiguous()
    out = torch.empty(fam.out_shape(len(zs), tuple(data.shape), geo), dtype=torch.complex64, device=data.device)
    for k in range(0, len(zs), max_z):
        fam.apply(data, wl, sp, zs[k:k + max_z], row, geo, out[k:k + max_z])
    return out


def asm_slice_apply(data, wavelengths, spacing, zs, row, pad_h, pad_w, unpad, bandlimit, out=None):
    """Raw launch of the z-x slice (thz_asm_slice_forward): data [B,C,H,W] complex64 -> [Z,B,C,Wo],
    output row ``row`` of every plane of ``zs`` (at most THZ_MAX_Z), equal to
    asm_apply(...)[:, :, :, row, :] without forming the planes.  Forward only; asm_propagate_zx is the
    differentiable form (backward: asm_slice_adjoint)."""
    return _slice_launch(_SLICE_FAMILIES["asm"], False, data, wavelengths, spacing, zs, row,
                         (pad_h, pad_w, unpad, bandlimit), None, out)


def asm_slice_adjoint(g, wavelengths, spacing, zs, row, pad_h, pad_w, unpad, bandlimit, height):
    """Raw launch of the z-x slice's adjoint (thz_asm_slice_adjoint): the cotangent g [Z,B,C,Wo]
    complex64 of asm_slice_apply(x [B,C,height,W], ..., row, ...) -> [B,C,height,W], the sum over the
    planes of each plane's adjoint -- asm_apply(g placed at row ``row`` of zero planes, adjoint=True)
    without forming the planes.  ``height`` is the field's H (g does not carry it).  At most
    THZ_MAX_Z planes."""
    return _slice_launch(_SLICE_FAMILIES["asm"], True, g, wavelengths, spacing, zs, row,
                         (pad_h, pad_w, unpad, bandlimit), height, None)


def asm_propagate_zx(data, wavelengths, spacing, zs, row, pad_h, pad_w, unpad=True, bandlimit="exact"):
    """Differentiable z-x slice on the slice kernels, forward and backward: [B,C,H,W] complex64 ->
    [Z,B,C,Wo], output row ``row`` of every plane of ``zs`` (any length: chunks of THZ_MAX_Z planes).
    The padded height must be one the slice kernels serve (asm_slice_native)."""
    return _slice_sweep(_SLICE_FAMILIES["asm"], data, wavelengths, spacing, zs, int(row),
                        (int(pad_h), int(pad_w), bool(unpad), _bandlimit(bandlimit)), True)


def czt_slice_apply(data, wavelengths, spacing, zs, row, outH, outW, odx, ody, out=None):
    """Raw launch of the CZT z-x slice (thz_czt_slice_forward): data [B,C,H,W] complex64 -> [Z,B,C,outH],
    output row ``row`` (the p of out[b, c, p, q]) of every plane of ``zs`` (at most THZ_MAX_Z), equal to
    czt_apply(..., z, ...)[:, :, row, :] per z without forming the planes.  Forward only;
    czt_propagate_zx is the differentiable form (backward: czt_slice_adjoint)."""
    return _slice_launch(_SLICE_FAMILIES["czt"], False, data, wavelengths, spacing, zs, row,
                         (outH, outW, odx, ody), None, out)


def czt_slice_adjoint(g, wavelengths, spacing, zs, row, outH, outW, odx, ody, field_hw, out=None):
    """Raw launch of the CZT z-x slice's adjoint (thz_czt_slice_adjoint): the cotangent g [Z,B,C,outH]
    complex64 of czt_slice_apply(x [B,C,H,W], ...) with (H, W) = field_hw -> [B,C,H,W], the sum over
    the planes of each plane's adjoint -- czt_apply(g placed at row ``row`` of a zero plane,
    adjoint=True) per z, summed, without forming a plane.  At most THZ_MAX_Z planes.  ``out``, when
    given, is a contiguous complex64 [B,C,H,W] tensor; every element of it is overwritten."""
    return _slice_launch(_SLICE_FAMILIES["czt"], True, g, wavelengths, spacing, zs, row,
                         (outH, outW, odx, ody), field_hw, out)


def czt_propagate_zx(data, wavelengths, spacing, zs, row, outH, outW, odx, ody):
    """Differentiable CZT z-x slice on the slice kernels, forward and backward: [B,C,H,W] complex64 ->
    [Z,B,C,outH], output row ``row`` of every plane of ``zs`` (any length: chunks of THZ_MAX_Z planes)."""
    return _slice_sweep(_SLICE_FAMILIES["czt"], data, wavelengths, spacing, zs, int(row),
                        (int(outH), int(outW), float(odx), float(ody)), True)


def rsc_slice_apply(data, wavelengths, spacing, zs, row, vectorial=False, out=None):
    """Raw launch of the RSC / VRS z-x slice (thz_rsc_slice_forward): data [B,C,H,W] complex64 ->
    [Z,Bo,C,Pw-W], output row ``row`` of every plane of ``zs`` (at most THZ_MAX_Z), equal to
    rsc_apply(..., z, vectorial)[:, :, row, :] per z without forming the planes or the kernel's
    2-D spectrum.  Forward only; rsc_propagate_zx is the differentiable form (backward:
    rsc_slice_adjoint)."""
    return _slice_launch(_SLICE_FAMILIES["rsc"], False, data, wavelengths, spacing, zs, row, (vectorial,), None, out)


def rsc_slice_adjoint(g, wavelengths, spacing, zs, row, field_shape, vectorial=False, out=None):
    """Raw launch of the RSC / VRS z-x slice's adjoint (thz_rsc_slice_adjoint): the cotangent g
    [Z,Bo,C,2(W//2)] complex64 of rsc_slice_apply(x, ...) with x.shape = field_shape = (B,C,H,W) ->
    [B,C,H,W], the sum over the planes of each plane's adjoint -- rsc_apply(g[k] placed at row ``row``
    of a zero plane, adjoint=True) per z, summed (VRS: with the Ez chain of each plane's own r), without
    forming a plane.  At most THZ_MAX_Z planes.  ``out``, when given, is a contiguous complex64
    [B,C,H,W] tensor; every element of it is overwritten."""
    return _slice_launch(_SLICE_FAMILIES["rsc"], True, g, wavelengths, spacing, zs, row, (vectorial,), field_shape,
                         out)


def rsc_propagate_zx(data, wavelengths, spacing, zs, row, vectorial=False):
    """Differentiable RSC / VRS z-x slice on the slice kernels, forward and backward: [B,C,H,W]
    complex64 -> [Z,Bo,C,2(W//2)], output row ``row`` of every plane of ``zs`` (any length: chunks of
    THZ_MAX_Z planes)."""
    return _slice_sweep(_SLICE_FAMILIES["rsc"], data, wavelengths, spacing, zs, int(row), (bool(vectorial),), True)
