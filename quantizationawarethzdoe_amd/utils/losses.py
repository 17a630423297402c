"""The reference's loss modules (utils/losses.py) on the fused kernels of csrc/thz_losses.hip.

``BinaryDiceLoss``, ``BinaryCEloss``, ``SSIMloss`` and ``Hierarchyloss`` keep the reference's
constructor arguments, defaults and ``forward(predict, target)`` signatures; the arithmetic runs in
``optics.dice_loss``, ``optics.bce_with_logits``, ``optics.ssim`` and ``optics.hierarchy_loss``
(float32 device tensors, differentiable in the prediction).  ``SSIMloss`` stands in for the
``pytorch_msssim.SSIM`` module the reference wraps and keeps its input checks.
"""
import torch
import torch.nn as nn

from .. import optics


class BinaryDiceLoss(nn.Module):
    """1 - (sum(p t) + smooth) / (sum(p^e) + sum(t^e) + smooth) per sample of [N, *] inputs, e = ``p``;
    reduction 'mean' / 'sum' over the batch or 'none' ([N])."""

    def __init__(self, smooth=1, p=2, reduction='mean'):
        super().__init__()
        self.smooth = smooth
        self.p = p
        self.reduction = reduction

    def forward(self, predict, target):
        assert predict.shape[0] == target.shape[0], "predict & target batch size don't match"
        if self.reduction not in ('mean', 'sum', 'none'):
            raise Exception('Unexpected reduction {}'.format(self.reduction))
        return optics.dice_loss(predict, target, smooth=self.smooth, p=self.p, reduction=self.reduction)


def _legacy_reduction(size_average, reduce, reduction):
    """torch's reading of the deprecated size_average / reduce pair (torch.nn._reduction)."""
    if size_average is None and reduce is None:
        return reduction
    if reduce is not None and not reduce:
        return 'none'
    return 'mean' if size_average is None or size_average else 'sum'


class BinaryCEloss(nn.Module):
    """Sigmoid + binary cross entropy in the numerically stable fused form (BCEWithLogitsLoss)."""

    def __init__(self, weight=None, size_average=None, reduce=None, reduction='mean', pos_weight=None) -> None:
        super().__init__()
        self.reduction = _legacy_reduction(size_average, reduce, reduction)
        self.register_buffer('weight', weight)
        self.register_buffer('pos_weight', pos_weight)

    def forward(self, predict, target):
        return optics.bce_with_logits(predict, target, weight=self.weight, pos_weight=self.pos_weight,
                                      reduction=self.reduction)


class SSIMloss(nn.Module):
    """1 - SSIM of [N, channel, H, W] images (Gaussian window of ``win_size`` taps, ``win_sigma``)."""

    def __init__(self, win_size=11, win_sigma=1.5, data_range=1, size_average=True, channel=1) -> None:
        super().__init__()
        if win_size % 2 != 1:
            raise ValueError('Window size should be odd.')
        self.win_size = win_size
        self.win_sigma = win_sigma
        self.data_range = data_range
        self.size_average = size_average
        self.channel = channel

    def forward(self, pred, target):
        if pred.shape != target.shape:
            raise ValueError(f'Input images should have the same dimensions, but got {pred.shape} and {target.shape}.')
        if pred.dim() == 5:
            raise NotImplementedError(f'SSIMloss: 3-D (5-d input) SSIM is not implemented; got {pred.shape}')
        if pred.dim() != 4:
            raise ValueError(f'Input images should be 4-d or 5-d tensors, but got {pred.shape}')
        if pred.shape[1] != self.channel:
            raise ValueError(f'SSIMloss: built for channel = {self.channel}, got an input with {pred.shape[1]} '
                             f'channels {tuple(pred.shape)}')
        return 1 - optics.ssim(pred, target, win_size=self.win_size, win_sigma=self.win_sigma,
                               data_range=self.data_range, size_average=self.size_average)


class Hierarchyloss(nn.Module):
    """BinaryCEloss + BinaryDiceLoss + SSIMloss at their defaults on the same prediction: the BCE term
    reads it as logits, the Dice and SSIM terms as a probability (the reference's own use)."""

    def __init__(self) -> None:
        super().__init__()
        self.bce = BinaryCEloss()
        self.dice = BinaryDiceLoss()
        self.ssimloss = SSIMloss()

    def forward(self, pred, ground_truth):
        assert pred.shape[0] == ground_truth.shape[0], "predict & target batch size don't match"
        if torch.is_tensor(pred) and pred.dim() == 4 and pred.shape[1] != self.ssimloss.channel:
            raise ValueError(f'SSIMloss: built for channel = {self.ssimloss.channel}, got an input with '
                             f'{pred.shape[1]} channels {tuple(pred.shape)}')
        return optics.hierarchy_loss(pred, ground_truth)
