"""The height-map helpers as plain torch ops, at any dtype and on any device.

Written from the formulas (the level index as a count of thresholds or the first minimum of the
distances; the surrogate slopes 0.5 s (1 - |z|)^(s - 1) 2 and sigma(s z) (1 - sigma(s z)) 4 s on
z = 2 (x - mid) / gap; the centred second difference scaled by W / 4 and H / 4 with a zero border), not
from the kernels.  tests/test_heightmap_cpu.py pins it to the reference's own outputs
(tests/golden/heightmap_golden.npz) and by identities; tests/test_heightmap_gpu.py holds the kernels to
its float64 evaluation.
"""
import torch
import torch.nn.functional as F


def _t(values, like):
    return torch.as_tensor(values, dtype=like.dtype, device=like.device)


def bucketize_idx(x, thresholds, wrap=False):
    """The number of thresholds not above x (a NaN x counts them all); wrap: modulo their number."""
    thr = _t(thresholds, x)
    idx = (~(thr > x.unsqueeze(-1))).sum(-1)
    return idx % len(thr) if wrap else idx


def argmin_idx(x, lut):
    """The first index of the smallest |x - lut[j]| (a NaN x gives 0)."""
    d = (x.unsqueeze(-1) - _t(lut, x)).abs()
    best = d.min(-1, keepdim=True).values
    hit = (d == best) | torch.isnan(d)
    return hit.int().argmax(-1)


def quantize(x, lut, thresholds=None, mode="bucketize", wrap=False):
    idx = argmin_idx(x, lut) if mode == "argmin" else bucketize_idx(x, thresholds, wrap)
    return _t(lut, x)[idx], idx


def slope(x, idx, lut, kind, s=1.0):
    """d q / d x as the surrogate ``kind`` defines it.  The other end of x's interval is the level
    beside lut[idx] on x's side, cyclically (below the first level: the last; above the last: the
    first); at x == lut[idx] it is the level itself, so z = 0."""
    if kind == "identity":
        return torch.ones_like(x)
    table = _t(lut, x)
    q = table[idx]
    side = torch.where(torch.isfinite(x - q), torch.sign(x - q), torch.zeros_like(x)).long()
    other = table[(idx + side) % len(table)]
    gap = (other - q).abs() + 1e-20
    z = 2 * (x - (other + q) / 2) / gap
    if kind == "poly":
        return torch.nan_to_num(0.5 * s * (1 - z.abs()) ** (s - 1)) * 2
    sg = torch.sigmoid(s * z)
    return sg * (1 - sg) * 4 * s


def center_difference(x):
    """dx, dy [..., H, W]: the interior of the zero-padded second difference, zero on the border."""
    H, W = x.shape[-2:]
    px = F.pad(x, (1, 1))
    py = F.pad(x, (0, 0, 1, 1))
    dx = W / 4 * (-px[..., :-2] + 2 * x - px[..., 2:])
    dy = H / 4 * (-py[..., :-2, :] + 2 * x - py[..., 2:, :])
    cols = torch.arange(W, device=x.device)
    rows = torch.arange(H, device=x.device).unsqueeze(-1)
    dx = torch.where((cols >= 1) & (cols <= W - 2), dx, torch.zeros_like(dx))
    dy = torch.where((rows >= 1) & (rows <= H - 2), dy, torch.zeros_like(dy))
    return dx, dy


def total_variation(x):
    dx, dy = center_difference(x)
    return dx.abs().mean() + dy.abs().mean()
