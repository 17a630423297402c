"""The four losses of utils/losses.py as plain torch ops, at any dtype and on any device.

Written from the published definitions (Dice: utils/losses.py:32-35; BCE with logits: torch's
documented formula; SSIM: Wang et al. 2004 with the Gaussian window, valid positions and constants
of pytorch_msssim), not from the kernels.  tests/test_losses_cpu.py pins it; tests/test_losses_gpu.py
holds the kernels to its float64 evaluation.
"""
import torch
import torch.nn.functional as F


def dice(pred, target, smooth=1, p=2, reduction="mean"):
    n = pred.shape[0]
    pr, tg = pred.reshape(n, -1), target.reshape(n, -1)
    num = (pr * tg).sum(1) + smooth
    den = (pr.pow(p) + tg.pow(p)).sum(1) + smooth
    return _reduce(1 - num / den, reduction)


def bce_map(x, t, weight=None, pos_weight=None):
    """Elementwise BCE with logits in the stable form."""
    sp = torch.log1p(torch.exp(-x.abs()))
    if weight is None and pos_weight is None:
        return x.clamp(min=0) - x * t + sp
    lw = 1 if pos_weight is None else 1 + (pos_weight - 1) * t
    out = (1 - t) * x + lw * (sp + (-x).clamp(min=0))
    return out if weight is None else out * weight


def bce(x, t, weight=None, pos_weight=None, reduction="mean"):
    return _reduce(bce_map(x, t, weight, pos_weight), reduction)


def _reduce(v, reduction):
    return v.mean() if reduction == "mean" else v.sum() if reduction == "sum" else v


def window(win_size, win_sigma, dtype=torch.float64, device=None):
    """exp(-(i - ws // 2)^2 / (2 sigma^2)), normalised, formed in ``dtype``."""
    coords = torch.arange(win_size, dtype=dtype, device=device) - win_size // 2
    g = torch.exp(-(coords ** 2) / (2 * win_sigma ** 2))
    return g / g.sum()


def _filter(v, win):
    """The separable window over the valid positions; an axis shorter than the window is not filtered."""
    C = v.shape[1]
    for axis in (2, 3):
        if v.shape[axis] < win.numel():
            continue
        shape = [C, 1, 1, 1]
        shape[axis] = win.numel()
        v = F.conv2d(v, win.reshape(1, 1, -1).expand(C, 1, -1).reshape(shape), groups=C, padding=0)
    return v


def ssim_moments(x, y, win):
    mx, my = _filter(x, win), _filter(y, win)
    return mx, my, _filter(x * x, win), _filter(y * y, win), _filter(x * y, win)


def ssim_map_from_moments(mx, my, mxx, myy, mxy, C1, C2):
    sx, sy, sxy = mxx - mx * mx, myy - my * my, mxy - mx * my
    A1, A2 = 2 * mx * my + C1, 2 * sxy + C2
    B1, B2 = mx * mx + my * my + C1, sx + sy + C2
    return A1 * A2 / (B1 * B2), (A1, A2, B1, B2)


def ssim_per_channel(x, y, win_size=11, win_sigma=1.5, data_range=1.0, K=(0.01, 0.03)):
    """[N, C]: the mean of the SSIM map over the valid window positions."""
    win = window(win_size, win_sigma, x.dtype, x.device)
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    S, _ = ssim_map_from_moments(*ssim_moments(x, y, win), C1, C2)
    return S.flatten(2).mean(-1)


def ssim(x, y, win_size=11, win_sigma=1.5, data_range=1.0, K=(0.01, 0.03), size_average=True,
         nonnegative_ssim=False):
    pc = ssim_per_channel(x, y, win_size, win_sigma, data_range, K)
    if nonnegative_ssim:
        pc = torch.relu(pc)
    return pc.mean() if size_average else pc.mean(1)


def ssim_grad_closed_form(x, y, g, win_size=11, win_sigma=1.5, data_range=1.0, K=(0.01, 0.03)):
    """d/dx of sum_nc g[n, c] ssim_per_channel[n, c] by the closed form: with a = dS/dmu_x, b = dS/dm_xx,
    c = dS/dm_xy per window position,
    grad_x = g / (H' W') ((w * a) + 2 x (w * b) + y (w * c)), * the adjoint of the valid filter."""
    win = window(win_size, win_sigma, x.dtype, x.device)
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    mx, my, mxx, myy, mxy = ssim_moments(x, y, win)
    S, (A1, A2, B1, B2) = ssim_map_from_moments(mx, my, mxx, myy, mxy, C1, C2)
    c = 2 * A1 / (B1 * B2)
    b = -S / B2
    a = 2 * my * (A2 - A1) / (B1 * B2) - 2 * mx * S * (1 / B1 - 1 / B2)

    def adjoint(v):
        C = v.shape[1]
        for axis in (2, 3):
            if x.shape[axis] < win.numel():
                continue
            shape = [C, 1, 1, 1]
            shape[axis] = win.numel()
            v = F.conv_transpose2d(v, win.reshape(1, 1, -1).expand(C, 1, -1).reshape(shape), groups=C)
        return v

    scale = g / (S.shape[2] * S.shape[3])
    return scale[:, :, None, None] * (adjoint(a) + 2 * x * adjoint(b) + y * adjoint(c))


def hierarchy(pred, target):
    return bce(pred, target) + dice(pred, target) + (1 - ssim(pred, target))
