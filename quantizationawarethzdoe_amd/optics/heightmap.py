"""Height-map helpers: the LUT quantizers with their surrogate gradients, center_difference and total_variation
(csrc/thz_heightmap.hip).  The torch op sequences the float64 paths run (``lut_forward_torch``,
``lut_slope_torch``, ``center_difference_torch``) are also what the tests and timing scripts compare against.
"""
import torch

from .. import _lib
from .._call import _require_device, call, workspace

LUT_MODES = {"bucketize": _lib.LUTQ_BUCKETIZE, "argmin": _lib.LUTQ_ARGMIN}
_LUT_KINDS = {"identity": _lib.LUTQ_GRAD_IDENTITY, "poly": _lib.LUTQ_GRAD_POLY, "sigmoid": _lib.LUTQ_GRAD_SIGMOID}


def host_table(values, who, dtype):
    """A table's values in x's precision as a tuple of host floats (they travel by value in the
    descriptor).  A list or a CPU tensor costs nothing on the device.  A device tensor is read back
    (a device-to-host copy that waits for the stream) on every call -- nothing is remembered, since
    neither a tensor's address nor its version pins its values -- and is refused while a graph is
    being captured, where such a read is not allowed."""
    if torch.is_tensor(values):
        t = values.detach().reshape(-1)
        if t.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{who}: a table given as a device tensor must be read back to the host, which a graph "
                               "capture does not allow; pass the table as a list or a CPU tensor")
        return tuple(t.to(dtype).tolist())
    try:
        return tuple(torch.tensor([float(v) for v in values], dtype=torch.float64).to(dtype).tolist())
    except TypeError:
        raise TypeError(f"{who}: the table must be a tensor or a sequence of numbers") from None


def lut_mid(lut, dtype):
    """lut_mid (utils/Helper_Functions.py:371-372) of the levels, in x's precision."""
    t = torch.tensor(lut, dtype=dtype)
    return tuple(((t[:-1] + t[1:]) / 2).tolist())


def lut_desc(n, mode, wrap, kind, lut, thr):
    d = _lib.LutQuantizeDesc(n=n, mode=mode, wrap=int(wrap), kind=kind, L=len(lut), T=len(thr))
    for i, v in enumerate(lut[:_lib.THZ_MAX_LUT]):
        d.lut[i] = v
    for i, v in enumerate(thr[:_lib.THZ_MAX_LUT]):
        d.thresholds[i] = v
    return d


def lut_forward_torch(x, lut, thr, mode, wrap):
    """The reference's op sequence: nearest_idx (utils/Helper_Functions.py:390-398) or the notebooks'
    argmin snap.  Returns (q, idx int64)."""
    lut_t = torch.tensor(lut, dtype=x.dtype, device=x.device)
    if mode == _lib.LUTQ_ARGMIN:
        idx = torch.argmin(torch.abs(x.unsqueeze(-1) - lut_t), dim=-1)
    else:
        idx = torch.bucketize(x, torch.tensor(thr, dtype=x.dtype, device=x.device), right=True)
        if wrap:
            idx = idx % len(thr)
    return lut_t[idx], idx


def lut_slope_torch(x, idx, lut, kind, s):
    """The surrogate slopes of Components/quantization.py:79-122 as torch ops, with the kernel's index
    rules (sign 0 when x - q is zero or not finite; idx + d taken modulo the number of levels)."""
    lut_t = torch.tensor(lut, dtype=x.dtype, device=x.device)
    q = lut_t[idx]
    dx = x - q
    d = torch.where(torch.isfinite(dx), torch.sign(dx), torch.zeros_like(dx)).long()
    other = lut_t[torch.remainder(idx + d, len(lut))]
    mid = (other + q) / 2
    gap = torch.abs(other - q) + 1e-20
    z = (x - mid) / gap * 2
    if kind == _lib.LUTQ_GRAD_POLY:
        return (0.5 * s * (1 - abs(z)) ** (s - 1)).nan_to_num() * 2.
    z = z * s
    return torch.sigmoid(z) * (1 - torch.sigmoid(z)) * (4. * s)


class _LutQuantize(torch.autograd.Function):
    """(q, idx int64) of a contiguous float32 / float64 device tensor; cfg = (mode, wrap, kind or None,
    lut, thresholds), s a device tensor [1] of x's dtype or None."""

    @staticmethod
    def forward(ctx, x, s, cfg):
        mode, wrap, kind, lut, thr = cfg
        if x.dtype == torch.float64:
            q, idx = lut_forward_torch(x, lut, thr, mode, wrap)
            idx32 = idx
        else:
            q = torch.empty_like(x)
            idx32 = torch.empty(x.shape, dtype=torch.int32, device=x.device)
            d = lut_desc(x.numel(), mode, wrap, 0, lut, thr)
            call(_lib.lib().thz_lut_quantize_forward, d, x, q, idx32, device=x.device)
            idx = idx32.long()
        ctx.mark_non_differentiable(idx)
        ctx.cfg = cfg
        if kind not in (None, _lib.LUTQ_GRAD_IDENTITY):
            ctx.save_for_backward(x, idx32, s)
        return q, idx

    @staticmethod
    def backward(ctx, g, _gidx):
        mode, wrap, kind, lut, thr = ctx.cfg
        if kind is None:
            return None, None, None
        if kind == _lib.LUTQ_GRAD_IDENTITY:  # Components/quantization.py:70-71 hands grad_output through
            return g, None, None
        x, idx32, s = ctx.saved_tensors
        g = g.to(x.dtype).contiguous()
        if x.dtype == torch.float64:
            return g * lut_slope_torch(x, idx32, lut, kind, s), None, None
        out = torch.empty_like(x)
        d = lut_desc(x.numel(), mode, wrap, kind, lut, ())
        call(_lib.lib().thz_lut_quantize_backward, d, x, idx32, g, s, out, device=x.device)
        return out, None, None


def _heightmap_input(x, who):
    if not torch.is_tensor(x):
        raise TypeError(f"{who}: the input must be a tensor")
    _require_device(x, who)
    if x.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{who}: kernels compute in float32 (float64 runs the torch op sequence); got {x.dtype}")
    return x.contiguous()


def lut_quantize(x, lut, *, mode="bucketize", wrap=False, midvals=None, surrogate="identity", s=1.0):
    """Snap ``x`` to the levels ``lut``: returns ``(q, idx)``, q = lut[idx] in x's shape and dtype, idx int64
    (not differentiable).

    ``mode="bucketize"``: nearest_neighbor_search / nearest_idx (utils/Helper_Functions.py:375-398):
    idx = torch.bucketize(x, midvals, right=True); ``midvals`` defaults to the float32 midpoints of
    neighbouring levels (lut_mid, :371-372) in x's precision and must ascend.  ``wrap=True`` then takes idx modulo
    len(midvals), the reference's own last step, which sends every x at or above the top threshold to
    level 0.  ``mode="argmin"``: the notebooks' ``quantization(input, lut)``: the first minimum of |x - lut|.
    Levels and thresholds are compared in float32 exactly as given: q and idx equal torch's bit for bit.

    ``surrogate``: the gradient handed to x -- "identity" (NearestNeighborSearch, Components/
    quantization.py:59-71), "poly" (:73-96), "sigmoid" (:98-122), or None for no gradient (the
    notebooks' post-hoc snap).  ``s`` is the steepness: a Python number, or a device tensor the
    backward kernel reads when it runs (a captured graph sees each replay's value).  Where the
    surrogates look up the "other end" lut[idx + sign(x - q)], index -1 reads the last level as in the
    reference, and an index one past the last level, where the reference raises, reads level 0.

    float32 tensors on the ROCm device run thz_lut_quantize_forward / _backward (one pass each);
    float64 device tensors run the reference's torch op sequence.  With ``lut`` and ``midvals`` given as
    lists or CPU tensors nothing syncs and the call is capturable in torch.cuda.graph.  A table given as
    a device tensor is read back to the host on every call (the levels travel by value in the kernel's
    descriptor): that waits for the stream, and inside a graph capture it raises RuntimeError."""
    who = "lut_quantize"
    if mode not in LUT_MODES:
        raise ValueError(f"{who}: mode must be 'bucketize' or 'argmin', got {mode!r}")
    if surrogate is not None and surrogate not in _LUT_KINDS:
        raise ValueError(f"{who}: surrogate must be 'identity', 'poly', 'sigmoid' or None, got {surrogate!r}")
    x = _heightmap_input(x, who)
    lut = host_table(lut, who, x.dtype)
    if not 1 <= len(lut) <= _lib.THZ_MAX_LUT:
        raise ValueError(f"{who}: {len(lut)} levels; the kernels take 1 .. {_lib.THZ_MAX_LUT}")
    thr = ()
    if mode == "bucketize":
        thr = lut_mid(lut, x.dtype) if midvals is None else host_table(midvals, who, x.dtype)
        lo, hi = (1, len(lut)) if wrap else (0, len(lut) - 1)
        if not lo <= len(thr) <= hi:
            raise ValueError(f"{who}: {len(thr)} thresholds for {len(lut)} levels (wrap={bool(wrap)}: {lo} .. {hi})")
    kind = None if surrogate is None else _LUT_KINDS[surrogate]
    s_dev = None
    if kind in (_lib.LUTQ_GRAD_POLY, _lib.LUTQ_GRAD_SIGMOID):
        if torch.is_tensor(s) and s.is_cuda:
            s_dev = s.detach().to(x.dtype).reshape(1)
        else:
            s_dev = torch.full((1,), float(s), dtype=x.dtype, device=x.device)
    cfg = (LUT_MODES[mode], bool(wrap), kind, lut, thr)
    if kind is None:
        with torch.no_grad():
            return _LutQuantize.apply(x.detach(), None, cfg)
    return _LutQuantize.apply(x, s_dev, cfg)


def center_difference_torch(x):
    """utils/Helper_Functions.py:56-70 on [N, H, W]."""
    dx, dy = torch.zeros_like(x), torch.zeros_like(x)
    _, H, W = x.shape
    dx[:, :, 1:-1] = W / 4 * (-x[:, :, 0:-2] + 2 * x[:, :, 1:-1] - x[:, :, 2:])
    dy[:, 1:-1, :] = H / 4 * (-x[:, 0:-2, :] + 2 * x[:, 1:-1, :] - x[:, 2:, :])
    return dx, dy


def _tv_backward(x, gdx, gdy, grad_loss, shape):
    N, H, W = shape
    grad = torch.empty(shape, dtype=torch.float32, device=(x if x is not None else gdx).device)
    call(_lib.lib().thz_tv_backward, x, gdx, gdy, grad_loss, N, H, W, grad, device=grad.device)
    return grad


class _CenterDifference(torch.autograd.Function):
    """dx, dy of a contiguous float32 [N, H, W]."""

    @staticmethod
    def forward(ctx, x):
        N, H, W = x.shape
        dx, dy = torch.empty_like(x), torch.empty_like(x)
        call(_lib.lib().thz_tv_forward, x, N, H, W, dx, dy, None, None, 0, device=x.device)
        ctx.shape = (N, H, W)
        return dx, dy

    @staticmethod
    def backward(ctx, gdx, gdy):
        return _tv_backward(None, gdx.float().contiguous(), gdy.float().contiguous(), None, ctx.shape)


class _TotalVariation(torch.autograd.Function):
    """mean |dx| + mean |dy| of a contiguous float32 [N, H, W], a 0-d tensor."""

    @staticmethod
    def forward(ctx, x):
        N, H, W = x.shape
        tv = torch.empty((), dtype=torch.float32, device=x.device)
        ws = workspace(_lib.lib().thz_tv_workspace_size, N, H, W, device=x.device)
        call(_lib.lib().thz_tv_forward, x, N, H, W, None, None, tv, ws, ws.numel(), device=x.device)
        ctx.save_for_backward(x)
        return tv

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        return _tv_backward(x, None, None, g.float().reshape(1), tuple(x.shape))


def as_planes(x, who):
    if x.dim() < 2:
        raise ValueError(f"{who}: the input needs the two spatial dimensions last; got shape {tuple(x.shape)}")
    if x.numel() == 0:
        raise ValueError(f"{who}: empty input {tuple(x.shape)}")
    return x.reshape(-1, x.shape[-2], x.shape[-1])


def center_difference(x):
    """center_difference (utils/Helper_Functions.py:56-70): ``(dx, dy)`` in x's shape,
    dx = W / 4 (-x[j-1] + 2 x[j] - x[j+1]) on the interior columns and 0 on the border, dy alike with H / 4
    on the interior rows (the last two dimensions are the spatial ones).  float32 on the ROCm device: one
    pass that reads x once and writes both maps (thz_tv_forward); the backward gathers the adjoint
    stencil of the two cotangents (thz_tv_backward).  float64 runs the torch op sequence."""
    x = _heightmap_input(x, "center_difference")
    p = as_planes(x, "center_difference")
    dx, dy = center_difference_torch(p) if x.dtype == torch.float64 else _CenterDifference.apply(p)
    return dx.reshape(x.shape), dy.reshape(x.shape)


def total_variation(x):
    """total_variation (utils/Helper_Functions.py:40-54): mean |dx| + mean |dy| of center_difference over
    every element, borders included, as a 0-d tensor; a 6-D [B, T, P, C, H, W] input is taken as
    [B T P, C, H, W] as the reference does.  float32 on the ROCm device: one pass that reads x once and
    forms the two sums as fp64 partials per workgroup added in a fixed order (thz_tv_forward; the same
    input gives the same bits); the backward recomputes sign(dx), sign(dy) from x and gathers their
    adjoint stencil, sign(0) = 0 (thz_tv_backward).  No host sync; float64 runs the torch op sequence."""
    x = _heightmap_input(x, "total_variation")
    p = as_planes(x, "total_variation")
    if x.dtype == torch.float64:
        dx, dy = center_difference_torch(p)
        return dx.abs().mean() + dy.abs().mean()
    return _TotalVariation.apply(p)
