"""The image losses of utils/losses.py -- Dice, BCE with logits, SSIM and their sum -- on fused streaming and
tile kernels (csrc/thz_losses.hip).
"""
import warnings

import torch

from .. import _lib
from .._call import _require_device, call, workspace


def _loss_pair(pred, target, who):
    """The checks every loss shares; returns the contiguous pair."""
    if not torch.is_tensor(pred) or not torch.is_tensor(target):
        raise TypeError(f"{who}: pred and target must be tensors")
    _require_device(pred, who)
    _require_device(target, who)
    if pred.dtype != torch.float32 or target.dtype != torch.float32:
        raise TypeError(f"{who}: kernels compute in float32; got {pred.dtype} and {target.dtype}")
    if target.requires_grad:
        raise NotImplementedError(f"{who}: the gradient with respect to target is not implemented; detach it")
    if pred.numel() == 0:
        raise ValueError(f"{who}: empty input {tuple(pred.shape)}")
    return pred.contiguous(), target.contiguous()


def _plane_like(w, pred, name):
    """weight / pos_weight expanded to pred's shape (torch broadcasts them; the kernel reads a plane)."""
    if w is None:
        return None
    w = torch.as_tensor(w, dtype=torch.float32, device=pred.device)
    if w.requires_grad:
        raise NotImplementedError(f"bce_with_logits: the gradient with respect to {name} is not implemented")
    return w.expand(pred.shape).contiguous()


def _dice_bce_desc(pred, terms, p=2.0, smooth=1.0, weight=None, pos_weight=None, elementwise=False):
    n = pred.shape[0] if pred.dim() else 1
    return _lib.DiceBceDesc(N=n, M=pred.numel() // n, p=float(p), smooth=float(smooth), terms=terms,
                            bce_grad_elementwise=int(elementwise),
                            weight=weight.data_ptr() if weight is not None else None,
                            pos_weight=pos_weight.data_ptr() if pos_weight is not None else None)


def _dice_bce_sums(pred, target, d, want_map=False):
    """sums [N, 4] float64 (sum p t, sum p^e, sum t^e, sum bce) and the BCE map or None."""
    sums = torch.empty((d.N, 4), dtype=torch.float64, device=pred.device)
    bmap = torch.empty_like(pred) if want_map else None
    ws = workspace(_lib.lib().thz_dice_bce_sums_workspace_size, d, device=pred.device)
    call(_lib.lib().thz_dice_bce_sums, d, pred, target, sums, bmap, ws, ws.numel(), device=pred.device)
    return sums, bmap


def _dice_bce_backward(pred, target, d, sums, g_dice, g_bce):
    grad = torch.empty_like(pred)
    call(_lib.lib().thz_dice_bce_backward, d, pred, target, sums, g_dice, g_bce, grad, device=pred.device)
    return grad


def _dice_from_sums(sums, smooth):
    """1 - num / den per sample (utils/losses.py:32-35) on the fp64 sums."""
    return 1 - (sums[:, 0] + smooth) / (sums[:, 1] + sums[:, 2] + smooth)


class _Dice(torch.autograd.Function):
    """The per-sample Dice loss [N] of contiguous pred, target."""

    @staticmethod
    def forward(ctx, pred, target, smooth, p):
        sums, _ = _dice_bce_sums(pred, target, _dice_bce_desc(pred, _lib.LOSS_TERM_DICE, p, smooth))
        ctx.save_for_backward(pred, target, sums)
        ctx.cfg = (smooth, p)
        return _dice_from_sums(sums, smooth).float()

    @staticmethod
    def backward(ctx, g):
        pred, target, sums = ctx.saved_tensors
        smooth, p = ctx.cfg
        d = _dice_bce_desc(pred, _lib.LOSS_TERM_DICE, p, smooth)
        return _dice_bce_backward(pred, target, d, sums, g.float().contiguous(), None), None, None, None


class _Bce(torch.autograd.Function):
    """BCE with logits of contiguous pred, target: the map (reduction 'none') or the sum times ``scale``."""

    @staticmethod
    def forward(ctx, pred, target, weight, pos_weight, reduction):
        none = reduction == "none"
        d = _dice_bce_desc(pred, _lib.LOSS_TERM_BCE, weight=weight, pos_weight=pos_weight)
        sums, bmap = _dice_bce_sums(pred, target, d, want_map=none)
        ctx.save_for_backward(pred, target, *(w for w in (weight, pos_weight) if w is not None))
        ctx.cfg = (weight is not None, pos_weight is not None, none,
                   1.0 / pred.numel() if reduction == "mean" else 1.0)
        return bmap if none else (sums[:, 3].sum() * ctx.cfg[3]).float()

    @staticmethod
    def backward(ctx, g):
        has_w, has_pw, none, scale = ctx.cfg
        pred, target, *planes = ctx.saved_tensors
        weight = planes.pop(0) if has_w else None
        pos_weight = planes.pop(0) if has_pw else None
        d = _dice_bce_desc(pred, _lib.LOSS_TERM_BCE, weight=weight, pos_weight=pos_weight, elementwise=none)
        g = g.float().contiguous() if none else (g.float() * scale).reshape(1)
        return _dice_bce_backward(pred, target, d, None, None, g), None, None, None, None


def _reduce(loss, reduction):
    if reduction == "mean":
        return loss.mean()
    if reduction == "sum":
        return loss.sum()
    if reduction == "none":
        return loss
    raise Exception("Unexpected reduction {}".format(reduction))


def dice_loss(pred, target, smooth=1, p=2, reduction="mean"):
    """BinaryDiceLoss (utils/losses.py:7-44): 1 - (sum p t + smooth) / (sum p^e + sum t^e + smooth) per
    sample of [N, *] inputs, then ``reduction``; one streaming pass forward (thz_dice_bce_sums), one
    backward (thz_dice_bce_backward), differentiable in ``pred``."""
    if reduction not in ("mean", "sum", "none"):
        raise Exception("Unexpected reduction {}".format(reduction))
    pred, target = _loss_pair(pred, target, "dice_loss")
    assert pred.shape[0] == target.shape[0], "predict & target batch size don't match"
    if pred.numel() != target.numel():
        raise ValueError(f"dice_loss: pred {tuple(pred.shape)} and target {tuple(target.shape)} differ in size")
    return _reduce(_Dice.apply(pred, target, float(smooth), float(p)), reduction)


def bce_with_logits(pred, target, weight=None, pos_weight=None, reduction="mean"):
    """torch.nn.BCEWithLogitsLoss (BinaryCEloss, utils/losses.py:47-58) in one streaming pass forward
    and one backward; ``weight`` / ``pos_weight`` broadcast to ``pred``; differentiable in ``pred``."""
    if reduction not in ("mean", "sum", "none"):
        raise ValueError(f"{reduction} is not a valid value for reduction")
    pred, target = _loss_pair(pred, target, "bce_with_logits")
    if pred.shape != target.shape:
        raise ValueError(f"Target size ({target.size()}) must be the same as input size ({pred.size()})")
    return _Bce.apply(pred, target, _plane_like(weight, pred, "weight"), _plane_like(pos_weight, pred, "pos_weight"),
                      reduction)


_ssim_windows = {}


def _ssim_window(win_size, win_sigma):
    """The 1-D Gaussian taps as pytorch_msssim forms them: float32 torch ops on the host."""
    key = (int(win_size), float(win_sigma))
    if key not in _ssim_windows:
        coords = torch.arange(key[0], dtype=torch.float32) - key[0] // 2
        g = torch.exp(-(coords ** 2) / (2 * key[1] ** 2))
        _ssim_windows[key] = tuple((g / g.sum()).tolist())
    return _ssim_windows[key]


def _ssim_desc(x, window, C1, C2, nonnegative=False, accumulate=False):
    N, C, H, W = x.shape
    d = _lib.SsimDesc(NC=N * C, H=H, W=W, ws=len(window), C1=C1, C2=C2, nonnegative=int(nonnegative),
                      accumulate=int(accumulate))
    for i, w in enumerate(window[:_lib.SSIM_MAX_WIN]):
        d.window[i] = w
    return d


def _ssim_forward(x, y, d, want_coef):
    """ssim [N, C] and the backward's coefficient planes [3, N, C, H', W'] or None."""
    N, C, H, W = x.shape
    out = torch.empty((N, C), dtype=torch.float32, device=x.device)
    coef = None
    if want_coef:
        wh, ww = (1 if H < d.ws else d.ws), (1 if W < d.ws else d.ws)
        coef = torch.empty((3, N, C, H - wh + 1, W - ww + 1), dtype=torch.float32, device=x.device)
    ws = workspace(_lib.lib().thz_ssim_workspace_size, d, device=x.device)
    call(_lib.lib().thz_ssim_forward, d, x, y, out, None, coef, ws, ws.numel(), device=x.device)
    return out, coef


def _ssim_backward(x, y, d, coef, out, g, grad):
    call(_lib.lib().thz_ssim_backward, d, x, y, coef, out, g, grad, device=x.device)
    return grad


class _Ssim(torch.autograd.Function):
    """ssim per (n, c) [N, C] of contiguous x, y [N, C, H, W]; cfg = (window, C1, C2, nonnegative)."""

    @staticmethod
    def forward(ctx, x, y, cfg):
        out, coef = _ssim_forward(x, y, _ssim_desc(x, *cfg), ctx.needs_input_grad[0])
        if coef is not None:
            ctx.save_for_backward(x, y, coef, out)
        ctx.cfg = cfg
        return out

    @staticmethod
    def backward(ctx, g):
        x, y, coef, out = ctx.saved_tensors
        grad = _ssim_backward(x, y, _ssim_desc(x, *ctx.cfg), coef, out, g.float().contiguous(), torch.empty_like(x))
        return grad, None, None


def _ssim_cfg(x, y, win_size, win_sigma, data_range, K, nonnegative_ssim, who):
    if x.shape != y.shape:
        raise ValueError(f"Input images should have the same dimensions, but got {x.shape} and {y.shape}.")
    if x.dim() == 5:
        raise NotImplementedError(f"{who}: 3-D (5-d input) SSIM is not implemented; got {x.shape}")
    if x.dim() != 4:
        raise ValueError(f"Input images should be 4-d or 5-d tensors, but got {x.shape}")
    if int(win_size) % 2 != 1:
        raise ValueError("Window size should be odd.")
    for i, n in enumerate(x.shape[2:]):
        if n < win_size:
            warnings.warn(f"Skipping Gaussian Smoothing at dimension 2+{i} for input: {x.shape} and win size: {win_size}")
    return (_ssim_window(win_size, win_sigma), (float(K[0]) * float(data_range)) ** 2,
            (float(K[1]) * float(data_range)) ** 2, bool(nonnegative_ssim))


def ssim(x, y, *, win_size=11, win_sigma=1.5, data_range=1.0, K=(0.01, 0.03), size_average=True,
         nonnegative_ssim=False):
    """pytorch_msssim.ssim (the measure behind SSIMloss, utils/losses.py:62-74) of [N, C, H, W] images:
    the mean over the valid window positions of the SSIM map, per (n, c), then the mean over all
    (a scalar) or over C ([N], ``size_average=False``).  One tiled kernel reads x and y once
    (thz_ssim_forward) and, when x needs a gradient, writes the three coefficient planes its backward
    gathers from (thz_ssim_backward); differentiable in ``x``."""
    cfg = _ssim_cfg(x, y, win_size, win_sigma, data_range, K, nonnegative_ssim, "ssim")
    x, y = _loss_pair(x, y, "ssim")
    per_channel = _Ssim.apply(x, y, cfg)
    return per_channel.mean() if size_average else per_channel.mean(1)


class _Hierarchy(torch.autograd.Function):
    """bce(pred, t) + dice(pred, t) + 1 - ssim(pred, t) with the references' defaults, all means."""

    @staticmethod
    def forward(ctx, pred, target, cfg):
        both = _lib.LOSS_TERM_DICE | _lib.LOSS_TERM_BCE
        sums, _ = _dice_bce_sums(pred, target, _dice_bce_desc(pred, both))
        out, coef = _ssim_forward(pred, target, _ssim_desc(pred, *cfg), ctx.needs_input_grad[0])
        if coef is not None:
            ctx.save_for_backward(pred, target, sums, coef, out)
        ctx.cfg = cfg
        loss = sums[:, 3].sum() / pred.numel() + _dice_from_sums(sums, 1.0).mean() + (1 - out.double().mean())
        return loss.float()

    @staticmethod
    def backward(ctx, g):
        pred, target, sums, coef, out = ctx.saved_tensors
        N, C = pred.shape[:2]
        g = g.float()
        d = _dice_bce_desc(pred, _lib.LOSS_TERM_DICE | _lib.LOSS_TERM_BCE)
        grad = _dice_bce_backward(pred, target, d, sums, (g / N).expand(N).contiguous(),
                                  (g / pred.numel()).reshape(1))
        gs = (-g / (N * C)).expand(N, C).contiguous()
        _ssim_backward(pred, target, _ssim_desc(pred, *ctx.cfg, accumulate=True), coef, out, gs, grad)
        return grad, None, None


def hierarchy_loss(pred, target):
    """Hierarchyloss (utils/losses.py:78-88): BinaryCEloss + BinaryDiceLoss + SSIMloss at their defaults
    on the same ``pred`` -- as logits for the BCE term and as a probability for Dice and SSIM, the
    reference's own use.  One thz_dice_bce_sums pass serves the Dice and BCE terms; the backward is one
    thz_dice_bce_backward pass plus the SSIM gather adding into the same gradient."""
    cfg = _ssim_cfg(pred, target, 11, 1.5, 1.0, (0.01, 0.03), False, "hierarchy_loss")
    pred, target = _loss_pair(pred, target, "hierarchy_loss")
    return _Hierarchy.apply(pred, target, cfg)
