"""utils.losses without a GPU: the reference-named module imports and constructs, the host-side
checks of the glue and of the C entries answer without a device, and tests/losses_ref.py -- the
float64 restatement the GPU tests hold the kernels to -- is pinned by identities of its own
(pytorch_msssim, which the reference's SSIMloss wraps, cannot be imported, so no reference-generated
fixture exists for this module)."""
import ctypes
import inspect

import pytest
import torch
import torch.nn.functional as F

import quantizationawarethzdoe_amd as pkg
from quantizationawarethzdoe_amd import _lib, optics
from tests import losses_ref as lr


# ---- the restatement ---------------------------------------------------------------------------
def _pair(shape, seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=dtype), torch.rand(shape, generator=g, dtype=dtype)


@pytest.mark.parametrize("ws,sigma", [(1, 1.5), (3, 0.5), (7, 1.0), (11, 1.5), (33, 5.0)])
def test_window_sums_to_one(ws, sigma):
    w = lr.window(ws, sigma)
    assert w.shape == (ws,) and abs(float(w.sum()) - 1) < 1e-15
    assert torch.equal(w, w.flip(0)) and int(w.argmax()) == ws // 2
    assert abs(float(lr.window(ws, sigma, torch.float32).double().sum()) - 1) < 3e-7


def test_ssim_of_identical_images_is_one():
    x, _ = _pair((2, 3, 20, 23))
    assert float((lr.ssim_per_channel(x, x) - 1).abs().max()) < 1e-14


@pytest.mark.parametrize("a,b", [(0.3, 0.7), (0.0, 1.0), (0.5, 0.5), (0.9, 0.25)])
def test_ssim_of_constant_images(a, b):
    x, y = torch.full((1, 2, 15, 17), a, dtype=torch.float64), torch.full((1, 2, 15, 17), b, dtype=torch.float64)
    C1 = 0.01 ** 2
    want = (2 * a * b + C1) / (a * a + b * b + C1)
    assert float((lr.ssim_per_channel(x, y) - want).abs().max()) < 1e-12
    assert abs(float(lr.ssim(x, y)) - want) < 1e-12


def test_ssim_skips_the_filter_along_a_short_axis():
    x, y = _pair((1, 1, 10, 30))
    got = lr.ssim_per_channel(x, y)
    win = lr.window(11, 1.5).reshape(1, 1, 1, 11)
    m = [F.conv2d(v, win) for v in (x, y, x * x, y * y, x * y)]
    S, _ = lr.ssim_map_from_moments(*m, 0.01 ** 2, 0.03 ** 2)
    assert S.shape == (1, 1, 10, 20) and float((got - S.mean()).abs()) < 1e-15


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_bce_equals_torch(weighted, reduction):
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(3, 1, 5, 7, generator=g, dtype=torch.float64) - 0.5) * 60
    t = torch.rand(3, 1, 5, 7, generator=g, dtype=torch.float64)
    w = torch.rand(3, 1, 5, 7, generator=g, dtype=torch.float64) + 0.5 if weighted else None
    pw = torch.rand(3, 1, 5, 7, generator=g, dtype=torch.float64) * 3 if weighted else None
    want = F.binary_cross_entropy_with_logits(x, t, weight=w, pos_weight=pw, reduction=reduction)
    got = lr.bce(x, t, w, pw, reduction)
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())
    if weighted:  # each plane alone
        for kw in (dict(weight=w), dict(pos_weight=pw)):
            want = F.binary_cross_entropy_with_logits(x, t, reduction=reduction, **kw)
            got = lr.bce(x, t, kw.get("weight"), kw.get("pos_weight"), reduction)
            assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())


def test_dice_of_the_definition():
    p, t = _pair((2, 7), seed=2)
    want = torch.stack([1 - ((p[i] * t[i]).sum() + 1) / ((p[i] ** 3).sum() + (t[i] ** 3).sum() + 1) for i in range(2)])
    assert float((lr.dice(p, t, p=3, reduction="none") - want).abs().max()) < 1e-15
    assert abs(float(lr.dice(p, p * 0 + 1, smooth=0, p=1)) - (1 - float(p[0].sum() / (p[0].sum() + 7)
                                                                     + p[1].sum() / (p[1].sum() + 7)) / 2)) < 1e-15


def test_ssim_closed_form_gradient_equals_autograd():
    x, y = _pair((1, 2, 13, 14), seed=3)
    g = torch.tensor([[0.7, -1.3]], dtype=torch.float64)
    xa = x.clone().requires_grad_(True)
    (lr.ssim_per_channel(xa, y) * g).sum().backward()
    got = lr.ssim_grad_closed_form(x, y, g)
    rel = float((got - xa.grad).norm() / xa.grad.norm())
    assert rel < 1e-10, rel


# ---- the module and the glue -------------------------------------------------------------------
def test_reference_import_path_and_construction():
    pkg.install_reference_aliases()
    from utils.losses import BinaryCEloss, BinaryDiceLoss, Hierarchyloss, SSIMloss
    d, b, s, h = BinaryDiceLoss(), BinaryCEloss(), SSIMloss(), Hierarchyloss()
    assert (d.smooth, d.p, d.reduction) == (1, 2, "mean")
    assert b.reduction == "mean" and b.weight is None and b.pos_weight is None
    assert (s.win_size, s.win_sigma, s.data_range, s.size_average, s.channel) == (11, 1.5, 1, True, 1)
    assert isinstance(h.bce, BinaryCEloss) and isinstance(h.dice, BinaryDiceLoss) and isinstance(h.ssimloss, SSIMloss)
    for cls, names in ((BinaryDiceLoss, ["smooth", "p", "reduction"]),
                       (BinaryCEloss, ["weight", "size_average", "reduce", "reduction", "pos_weight"]),
                       (SSIMloss, ["win_size", "win_sigma", "data_range", "size_average", "channel"]),
                       (Hierarchyloss, [])):
        assert list(inspect.signature(cls.__init__).parameters)[1:] == names
    assert list(inspect.signature(Hierarchyloss.forward).parameters) == ["self", "pred", "ground_truth"]
    assert list(inspect.signature(BinaryDiceLoss.forward).parameters) == ["self", "predict", "target"]
    assert BinaryCEloss(reduce=False).reduction == "none" and BinaryCEloss(size_average=False).reduction == "sum"
    assert list(BinaryCEloss(pos_weight=torch.ones(3)).state_dict()) == ["pos_weight"]


def test_host_side_errors():
    from quantizationawarethzdoe_amd.utils.losses import BinaryCEloss, BinaryDiceLoss, Hierarchyloss, SSIMloss
    x = torch.rand(2, 1, 16, 16)
    with pytest.raises(Exception, match="Unexpected reduction batch"):
        BinaryDiceLoss(reduction="batch")(x, x)
    with pytest.raises(AssertionError, match="batch size don't match"):
        BinaryDiceLoss()(x, x[:1])
    with pytest.raises(ValueError, match="Window size should be odd"):
        SSIMloss(win_size=10)
    with pytest.raises(ValueError, match="Window size should be odd"):
        optics.ssim(x, x, win_size=8)
    with pytest.raises(ValueError, match="channel"):
        SSIMloss(channel=3)(x, x)
    with pytest.raises(ValueError, match="channel"):
        Hierarchyloss()(x.expand(2, 3, 16, 16), x.expand(2, 3, 16, 16))
    with pytest.raises(ValueError, match="should have the same dimensions"):
        SSIMloss()(x, x[:, :, :8])
    with pytest.raises(NotImplementedError, match="5-d"):
        SSIMloss()(x[None], x[None])
    with pytest.raises(ValueError, match="4-d or 5-d"):
        SSIMloss()(x[0], x[0])
    # no CPU compute path
    for call in (lambda: BinaryDiceLoss()(x, x), lambda: BinaryCEloss()(x, x), lambda: SSIMloss()(x, x),
                 lambda: Hierarchyloss()(x, x), lambda: optics.ssim(x, x), lambda: optics.hierarchy_loss(x, x),
                 lambda: optics.dice_loss(x, x), lambda: optics.bce_with_logits(x, x)):
        with pytest.raises(RuntimeError, match="ROCm device"):
            call()


L = ctypes.c_void_p(0)
P8 = ctypes.c_void_p(256)  # a non-null, aligned address no entry dereferences on the host


def _err():
    return _lib.lib().thz_last_error().decode()


def _ssim_desc(ws=11, H=16, W=16, NC=1):
    return _lib.SsimDesc(NC=NC, H=H, W=W, ws=ws, C1=1e-4, C2=9e-4)


def _ssim_calls(d):
    h, n = _lib.lib(), ctypes.c_size_t(0)
    return (lambda: h.thz_ssim_workspace_size(ctypes.byref(d), ctypes.byref(n)),
            lambda: h.thz_ssim_forward(ctypes.byref(d), P8, P8, P8, L, L, P8, 1 << 20, L),
            lambda: h.thz_ssim_backward(ctypes.byref(d), P8, P8, P8, P8, P8, P8, L))


@pytest.mark.parametrize("ws", [35, 10, 0, 2, -3])
def test_ssim_entries_refuse_the_window(ws):
    for call in _ssim_calls(_ssim_desc(ws=ws)):
        assert call() == _lib.THZ_E_UNSUPPORTED
        assert "window" in _err() and str(ws) in _err()


@pytest.mark.parametrize("kw", [dict(H=0), dict(W=0), dict(NC=0), dict(H=-4)])
def test_ssim_entries_refuse_the_shape(kw):
    for call in _ssim_calls(_ssim_desc(**kw)):
        assert call() == _lib.THZ_E_ARG and "bad shape" in _err()


def test_ssim_entries_refuse_null_pointers():
    h, d, n = _lib.lib(), _ssim_desc(), ctypes.c_size_t(0)
    assert h.thz_ssim_workspace_size(None, ctypes.byref(n)) == _lib.THZ_E_ARG and "null" in _err()
    assert h.thz_ssim_workspace_size(ctypes.byref(d), None) == _lib.THZ_E_ARG and "null" in _err()
    assert h.thz_ssim_workspace_size(ctypes.byref(d), ctypes.byref(n)) == _lib.THZ_OK and n.value >= 16
    assert h.thz_ssim_forward(None, P8, P8, P8, L, L, P8, 1 << 20, L) == _lib.THZ_E_ARG
    for hole in range(3):
        args = [P8, P8, P8]
        args[hole] = L
        assert h.thz_ssim_forward(ctypes.byref(d), *args, L, L, P8, 1 << 20, L) == _lib.THZ_E_ARG and "null" in _err()
    assert h.thz_ssim_forward(ctypes.byref(d), P8, P8, P8, L, L, L, 0, L) == _lib.THZ_E_ARG
    assert h.thz_ssim_forward(ctypes.byref(d), P8, P8, P8, L, L, P8, 8, L) == _lib.THZ_E_WORKSPACE
    assert h.thz_ssim_backward(None, P8, P8, P8, P8, P8, P8, L) == _lib.THZ_E_ARG
    for hole in range(6):
        args = [P8] * 6
        args[hole] = L
        assert h.thz_ssim_backward(ctypes.byref(d), *args, L) == _lib.THZ_E_ARG and "null" in _err()


def _db_desc(N=2, M=8, terms=3, **kw):
    return _lib.DiceBceDesc(N=N, M=M, p=2.0, smooth=1.0, terms=terms, **kw)


def test_dice_bce_entries_refuse_bad_arguments():
    h, n = _lib.lib(), ctypes.c_size_t(0)
    for d in (_db_desc(N=0), _db_desc(M=0), _db_desc(M=-1)):
        assert h.thz_dice_bce_sums_workspace_size(ctypes.byref(d), ctypes.byref(n)) == _lib.THZ_E_ARG
        assert "bad shape" in _err()
        assert h.thz_dice_bce_sums(ctypes.byref(d), P8, P8, P8, L, P8, 1 << 20, L) == _lib.THZ_E_ARG
        assert h.thz_dice_bce_backward(ctypes.byref(d), P8, P8, P8, P8, P8, P8, L) == _lib.THZ_E_ARG
    for terms in (0, 4, 7):
        d = _db_desc(terms=terms)
        assert h.thz_dice_bce_sums(ctypes.byref(d), P8, P8, P8, L, P8, 1 << 20, L) == _lib.THZ_E_ARG and "terms" in _err()
    big = _db_desc(N=(1 << 24) + 1)
    assert h.thz_dice_bce_sums_workspace_size(ctypes.byref(big), ctypes.byref(n)) == _lib.THZ_E_UNSUPPORTED
    d = _db_desc()
    assert h.thz_dice_bce_sums_workspace_size(None, ctypes.byref(n)) == _lib.THZ_E_ARG
    assert h.thz_dice_bce_sums_workspace_size(ctypes.byref(d), None) == _lib.THZ_E_ARG
    assert h.thz_dice_bce_sums_workspace_size(ctypes.byref(d), ctypes.byref(n)) == _lib.THZ_OK and n.value >= 64
    assert h.thz_dice_bce_sums(None, P8, P8, P8, L, P8, 1 << 20, L) == _lib.THZ_E_ARG
    for hole in range(3):
        args = [P8, P8, P8]
        args[hole] = L
        assert h.thz_dice_bce_sums(ctypes.byref(d), *args, L, P8, 1 << 20, L) == _lib.THZ_E_ARG and "null" in _err()
    assert h.thz_dice_bce_sums(ctypes.byref(d), P8, P8, P8, L, L, 0, L) == _lib.THZ_E_ARG
    assert h.thz_dice_bce_sums(ctypes.byref(d), P8, P8, P8, L, P8, 8, L) == _lib.THZ_E_WORKSPACE
    dice_only = _db_desc(terms=_lib.LOSS_TERM_DICE)
    assert h.thz_dice_bce_sums(ctypes.byref(dice_only), P8, P8, P8, P8, P8, 1 << 20, L) == _lib.THZ_E_ARG
    assert h.thz_dice_bce_backward(None, P8, P8, P8, P8, P8, P8, L) == _lib.THZ_E_ARG
    for hole in range(6):
        args = [P8] * 6
        args[hole] = L
        assert h.thz_dice_bce_backward(ctypes.byref(d), *args, L) == _lib.THZ_E_ARG and "null" in _err()
    assert h.thz_dice_bce_backward(ctypes.byref(d), P8, ctypes.c_void_p(258), P8, P8, P8, P8, L) == _lib.THZ_E_ARG


def test_new_entries_are_exported():
    names = {"thz_dice_bce_sums_workspace_size", "thz_dice_bce_sums", "thz_dice_bce_backward",
             "thz_ssim_workspace_size", "thz_ssim_forward", "thz_ssim_backward"}
    h = _lib.lib()
    assert names <= set(_lib.EXPORTED) and all(hasattr(h, n) for n in names)
