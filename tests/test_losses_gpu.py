"""The loss kernels on the GPU (thz_losses.hip through optics.dice_loss / bce_with_logits / ssim /
hierarchy_loss and the reference-named modules of utils.losses).

Bound.  The reference is tests/losses_ref.py in float64 on the CPU (pinned by tests/test_losses_cpu.py).
For every compared quantity
    |kernel - fp64| <= 4 x max(e32, 2^-24 |value|),
e32 the error of the same restatement in float32 on the CPU on the same input, 4 the project's
table-parity factor, the floor one rounding of the output.  A quantity with many
elements (a reduction='none' output, a size_average=False vector) is compared in the maximum norm:
err, e32 and |value| are the maxima over its elements -- an element the float32 sequence happens to
get exactly must not turn the floor into a per-element demand of one rounding on a map whose every
element carries several.  Gradients: relative L2 against the float64 autograd of the restatement,
<= 4 x max(e32, 1e-6), as the Stokes backward test.

Every comparison prints its ratio err / bound; THZ_LOSSES_PARITY_LOG=<file> writes the largest per
loss there (profiles/losses_parity_ratios.txt is such a run on an MI355X).
"""
import os
import warnings

import pytest
import torch

from quantizationawarethzdoe_amd import _lib, optics
from quantizationawarethzdoe_amd.utils import losses as M
from tests import losses_ref as lr

pytestmark = pytest.mark.gpu

RATIOS = {}


def _dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _ratio_log():
    yield
    path = os.environ.get("THZ_LOSSES_PARITY_LOG")
    if path:
        with open(path, "w") as fh:
            fh.write("# largest err / bound per loss; bound = 4 max(e32, 2^-24 |value|) (values), "
                     "4 max(e32, 1e-6) (gradients, relative L2)\n")
            for k in sorted(RATIOS):
                fh.write(f"{k:28s} {RATIOS[k][0]:.4f}   ({RATIOS[k][1]})\n")


def _note(loss, case, ratio):
    print(f"{loss:24s} {case:60s} err / bound = {ratio:.4f}")
    if loss not in RATIOS or ratio > RATIOS[loss][0]:
        RATIOS[loss] = (ratio, case)


def _value(loss, case, got, fn):
    """fn(dtype) -> the restatement on the CPU.  Maximum norm over the quantity's elements."""
    r64, r32 = fn(torch.float64), fn(torch.float32)
    got = got.detach().cpu().double()
    assert got.shape == r64.shape, (got.shape, r64.shape)
    assert bool(torch.isfinite(got).all())
    err = float((got - r64).abs().max())
    e32 = float((r32.double() - r64).abs().max())
    bound = 4 * max(e32, 2.0 ** -24 * float(r64.abs().max()))
    _note(loss, case, err / bound if bound else float(err > 0))
    assert err <= bound, (loss, case, err, e32, bound)


def _grad(loss, case, got, fn):
    """fn(dtype) -> the gradient of the restatement by autograd on the CPU.  Relative L2."""
    g64, g32 = fn(torch.float64), fn(torch.float32)
    got = got.detach().cpu().double()
    assert got.shape == g64.shape and bool(torch.isfinite(got).all())
    nrm = float(g64.norm())
    if nrm == 0:
        assert float(got.abs().max()) == 0
        return
    err, e32 = float((got - g64).norm()) / nrm, float((g32.double() - g64).norm()) / nrm
    bound = 4 * max(e32, 1e-6)
    _note(loss + " grad", case, err / bound)
    assert err <= bound, (loss, case, err, e32, bound)


def _autograd(f, x, *rest):
    """dtype -> d f(x, *rest) / dx on the CPU in that dtype."""
    def run(dtype):
        xa = x.detach().to(dtype).clone().requires_grad_(True)
        f(xa, *(r.to(dtype) if torch.is_tensor(r) and r.is_floating_point() else r for r in rest)).backward()
        return xa.grad
    return run


def _place(t, offset=0):
    """A contiguous device copy whose pointer is 16-byte aligned (offset 0) or one element past."""
    buf = torch.empty(t.numel() + offset, dtype=t.dtype, device=_dev())
    v = buf[offset:].view(t.shape)
    v.copy_(t)
    assert (v.data_ptr() % 16 == 0) == (offset == 0)
    return v.detach()


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


# ---- SSIM forward ------------------------------------------------------------------------------
SSIM_SHAPES = [(1, 1, 11, 11, 11, 1.5), (2, 3, 11, 40, 11, 1.5), (1, 1, 12, 11, 11, 1.5), (1, 2, 97, 130, 11, 1.5),
               (2, 1, 33, 35, 3, 0.5), (1, 1, 40, 47, 7, 1.0), (1, 1, 67, 70, 33, 5.0), (1, 1, 10, 64, 11, 1.5)]
SSIM_INPUTS = ["uniform", "noisy", "constant", "edge"]


def _images(kind, shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    N, C, H, W = shape
    if kind == "uniform":
        x, y = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    elif kind == "noisy":
        x = torch.rand(shape, generator=g)
        y = (x + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1)
    elif kind == "constant":
        x = torch.full(shape, 0.3) + 0.1 * torch.arange(N * C).reshape(N, C, 1, 1)
        y = torch.full(shape, 0.7) - 0.05 * torch.arange(N * C).reshape(N, C, 1, 1)
    else:
        x = torch.zeros(shape)
        x[..., W // 2:] = 1.0
        y = torch.zeros(shape)
        y[..., H // 2:, :] = 0.8
        y[..., : W // 3] += 0.1
    return x * scale, y * scale


@pytest.mark.parametrize("kind", SSIM_INPUTS)
@pytest.mark.parametrize("shape", SSIM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ssim_forward(shape, kind):
    *dims, ws, sigma = shape
    x, y = _images(kind, tuple(dims))
    skipped = dims[2] < ws or dims[3] < ws
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        got = optics.ssim(x.to(_dev()), y.to(_dev()), win_size=ws, win_sigma=sigma)
        vec = optics.ssim(x.to(_dev()), y.to(_dev()), win_size=ws, win_sigma=sigma, size_average=False)
    assert any("Skipping Gaussian Smoothing" in str(w.message) for w in seen) == skipped
    case = f"{shape} {kind}"
    _value("ssim", case, got, lambda dt: lr.ssim(x.to(dt), y.to(dt), ws, sigma))
    _value("ssim", case + " [N]", vec, lambda dt: lr.ssim(x.to(dt), y.to(dt), ws, sigma, size_average=False))
    assert got.shape == () and vec.shape == (dims[0],)


def test_ssim_options():
    x, y = _images("noisy", (2, 2, 40, 37), scale=255.0)
    got = optics.ssim(x.to(_dev()), y.to(_dev()), data_range=255)
    _value("ssim", "data_range 255", got, lambda dt: lr.ssim(x.to(dt), y.to(dt), data_range=255.0))
    got = optics.ssim(x.to(_dev()), y.to(_dev()), data_range=255, K=(0.02, 0.05), win_size=5, win_sigma=0.8)
    _value("ssim", "K, window", got,
           lambda dt: lr.ssim(x.to(dt), y.to(dt), 5, 0.8, data_range=255.0, K=(0.02, 0.05)))
    x, y = _anticorrelated()
    assert float(lr.ssim_per_channel(x.double(), y.double())[0, 0]) < -0.05
    for size_average in (True, False):
        got = optics.ssim(x.to(_dev()), y.to(_dev()), nonnegative_ssim=True, size_average=size_average)
        _value("ssim", f"nonnegative size_average={size_average}", got,
               lambda dt: lr.ssim(x.to(dt), y.to(dt), nonnegative_ssim=True, size_average=size_average))
    m = M.SSIMloss(channel=2, size_average=False)(x.to(_dev()), y.to(_dev()))
    _value("ssim", "SSIMloss module", m, lambda dt: 1 - lr.ssim(x.to(dt), y.to(dt), size_average=False))


def _anticorrelated():
    """[2, 2, 24, 29]: channel 0 of every sample against its own negative image (mean SSIM < 0),
    channel 1 against a noisy copy."""
    g = torch.Generator().manual_seed(11)
    x = torch.rand(2, 2, 24, 29, generator=g)
    y = x.clone()
    y[:, 0] = 1 - x[:, 0]
    y[:, 1] = (x[:, 1] + 0.05 * torch.randn(2, 24, 29, generator=g)).clamp(0, 1)
    return x, y


# ---- Dice / BCE --------------------------------------------------------------------------------
DB_SHAPES = [((1, 1), 0), ((2, 7), 0), ((3, 1, 5, 7), 0), ((3, 1, 5, 7), 1), ((2, 1, 64, 64), 0), ((2, 3000), 0)]


def _logits(shape, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    x = (torch.rand(shape, generator=g) - 0.5) * 60
    t = torch.rand(shape, generator=g)
    w = torch.rand(shape, generator=g) + 0.5
    pw = torch.rand(shape[-1:], generator=g) * 3 + 0.2  # broadcast by the glue
    return x, t, w, pw


@pytest.mark.parametrize("shape,offset", DB_SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_dice_bce_forward(shape, offset):
    x, t, w, pw = _logits(shape)
    prob = torch.sigmoid(x / 10)
    dx, dt_, dw, dprob = (_place(v, offset) for v in (x, t, w, prob))
    for red in ("mean", "sum", "none"):
        for p in (1, 2, 3):
            for pred, dpred, tag in ((prob, dprob, "prob"), (x, dx, "logits")):
                got = optics.dice_loss(dpred, dt_, smooth=1, p=p, reduction=red)
                _value("dice", f"{shape}+{offset} p={p} {red} {tag}", got,
                       lambda dt: lr.dice(pred.to(dt), t.to(dt), 1, p, red))
        got = optics.bce_with_logits(dx, dt_, reduction=red)
        _value("bce", f"{shape}+{offset} {red}", got, lambda dt: lr.bce(x.to(dt), t.to(dt), reduction=red))
        for kw, kd in ((dict(weight=w), dict(weight=dw)), (dict(pos_weight=pw), dict(pos_weight=pw.to(_dev()))),
                       (dict(weight=w, pos_weight=pw), dict(weight=dw, pos_weight=pw.to(_dev())))):
            got = optics.bce_with_logits(dx, dt_, reduction=red, **kd)
            _value("bce", f"{shape}+{offset} {red} {sorted(kw)}", got,
                   lambda dt: lr.bce(x.to(dt), t.to(dt), reduction=red, **{k: v.to(dt) for k, v in kw.items()}))
    got = M.BinaryDiceLoss(smooth=0.5, p=2, reduction="sum")(dprob, dt_)
    _value("dice", f"{shape}+{offset} module", got, lambda dt: lr.dice(prob.to(dt), t.to(dt), 0.5, 2, "sum"))
    got = M.BinaryCEloss(pos_weight=pw).to(_dev())(dx, dt_)
    _value("bce", f"{shape}+{offset} module", got, lambda dt: lr.bce(x.to(dt), t.to(dt), pos_weight=pw.to(dt)))
    # log1p(exp(-|x|)) underflows at the ends of the range and nothing overflows
    ends = torch.tensor([[30.0, -30.0, 30.0, -30.0, 0.0]])
    tt = torch.tensor([[1.0, 1.0, 0.0, 0.0, 0.5]])
    got = optics.bce_with_logits(ends.to(_dev()), tt.to(_dev()), reduction="none")
    _value("bce", "ends of the range", got, lambda dt: lr.bce_map(ends.to(dt), tt.to(dt)))


# ---- backward ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,offset", [((3, 1, 5, 7), 1), ((3, 1, 5, 7), 0), ((2, 3000), 0)],
                         ids=lambda v: str(v).replace(" ", ""))
def test_dice_bce_backward(shape, offset):
    x, t, w, pw = _logits(shape, seed=1)
    prob = torch.sigmoid(x / 10)
    up = torch.rand(shape[0]) + 0.5
    for p in (1, 2, 3):
        for red in ("mean", "none"):
            dp = _place(prob, offset).requires_grad_(True)
            out = optics.dice_loss(dp, _place(t, offset), p=p, reduction=red)
            (out * up.to(_dev())).sum().backward() if red == "none" else out.backward()
            f = (lambda a, b: (lr.dice(a, b, 1, p, "none") * up.to(a.dtype)).sum()) if red == "none" else \
                (lambda a, b: lr.dice(a, b, 1, p, "mean"))
            _grad("dice", f"{shape}+{offset} p={p} {red}", dp.grad, _autograd(f, prob, t))
    upm = torch.rand(shape) + 0.5
    for kw in ({}, dict(weight=w, pos_weight=pw), dict(pos_weight=pw)):
        for red in ("mean", "sum", "none"):
            dx = _place(x, offset).requires_grad_(True)
            out = optics.bce_with_logits(dx, _place(t, offset), reduction=red,
                                         **{k: v.to(_dev()) for k, v in kw.items()})
            (out * upm.to(_dev())).sum().backward() if red == "none" else out.backward()

            def f(a, b, red=red, kw=kw):
                v = lr.bce(a, b, reduction=red, **{k: u.to(a.dtype) for k, u in kw.items()})
                return (v * upm.to(a.dtype)).sum() if red == "none" else v
            _grad("bce", f"{shape}+{offset} {red} {sorted(kw)}", dx.grad, _autograd(f, x, t))
            assert dx.grad.shape == dx.shape


@pytest.mark.parametrize("shape", [(1, 2, 97, 130, 11, 1.5), (1, 1, 11, 11, 11, 1.5), (1, 1, 67, 70, 33, 5.0),
                                   (1, 1, 10, 64, 11, 1.5), (2, 1, 33, 35, 3, 0.5)],
                         ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", ["uniform", "noisy"])
def test_ssim_backward(shape, kind):
    *dims, ws, sigma = shape
    x, y = _images(kind, tuple(dims), seed=5)
    dx = x.to(_dev()).requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        optics.ssim(dx, y.to(_dev()), win_size=ws, win_sigma=sigma).backward()
    _grad("ssim", f"{shape} {kind}", dx.grad, _autograd(lambda a, b: lr.ssim(a, b, ws, sigma), x, y))
    # size_average=False under a non-uniform upstream gradient
    up = torch.tensor([1.5, -0.25])[: dims[0]]
    dx = x.to(_dev()).requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        (optics.ssim(dx, y.to(_dev()), win_size=ws, win_sigma=sigma, size_average=False) * up.to(_dev())).sum().backward()
    _grad("ssim", f"{shape} {kind} [N] weighted", dx.grad,
          _autograd(lambda a, b: (lr.ssim(a, b, ws, sigma, size_average=False) * up.to(a.dtype)).sum(), x, y))


def test_ssim_backward_nonnegative_gates_the_negative_channel():
    x, y = _anticorrelated()
    dx = x.to(_dev()).requires_grad_(True)
    up = torch.tensor([2.0, -0.5])
    (optics.ssim(dx, y.to(_dev()), nonnegative_ssim=True, size_average=False) * up.to(_dev())).sum().backward()
    assert float(dx.grad[:, 0].abs().max()) == 0 and float(dx.grad[:, 1].abs().min()) > 0
    _grad("ssim", "nonnegative", dx.grad,
          _autograd(lambda a, b: (lr.ssim(a, b, nonnegative_ssim=True, size_average=False) * up.to(a.dtype)).sum(), x, y))
    t = y.to(_dev()).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="target"):
        optics.ssim(x.to(_dev()), t)
    with pytest.raises(TypeError, match="float32"):
        optics.ssim(x.to(_dev()).double(), y.to(_dev()).double())


# ---- Hierarchyloss -----------------------------------------------------------------------------
def _hier_inputs(shape, seed=7):
    g = torch.Generator().manual_seed(seed)
    t = (torch.rand(shape, generator=g) > 0.6).float()
    return (0.7 * t + 0.3 * torch.rand(shape, generator=g)), t


def _fwd_bwd(fn, x, t):
    dx = x.clone().requires_grad_(True)
    out = fn(dx, t)
    out.backward()
    return out.detach(), dx.grad


@pytest.mark.parametrize("shape", [(2, 1, 43, 75), (1, 1, 11, 11)], ids=str)
def test_hierarchy_loss(shape):
    x, t = _hier_inputs(shape)
    dx, dt_ = x.to(_dev()), t.to(_dev())
    _lib.timing_enable(True)
    try:
        _lib.timing_reset()
        dxg = dx.clone().requires_grad_(True)
        out = M.Hierarchyloss()(dxg, dt_)
        torch.cuda.synchronize()
        launches = {k: _lib.timing_read(k)[1] for k in ("dice_bce_sums", "dice_bce_finish", "ssim_fwd", "dice_bce_bwd",
                                                        "ssim_bwd")}
        assert launches == dict(dice_bce_sums=1, dice_bce_finish=1, ssim_fwd=1, dice_bce_bwd=0, ssim_bwd=0), launches
        out.backward()
        torch.cuda.synchronize()
        assert _lib.timing_read("dice_bce_bwd")[1] == 1 and _lib.timing_read("ssim_bwd")[1] == 1
        assert _lib.timing_read("dice_bce_sums")[1] == 1
    finally:
        _lib.timing_enable(False)
    _value("hierarchy", f"{shape}", out, lambda dt: lr.hierarchy(x.to(dt), t.to(dt)))
    _grad("hierarchy", f"{shape}", dxg.grad, _autograd(lr.hierarchy, x, t))
    # the three terms computed separately by the kernels: the same value and gradient
    parts, pgrad = _fwd_bwd(lambda a, b: optics.bce_with_logits(a, b) + optics.dice_loss(a, b) + (1 - optics.ssim(a, b)),
                            dx, dt_)
    ref64 = lr.hierarchy(x.double(), t.double())
    e32 = abs(float(lr.hierarchy(x, t)) - float(ref64))
    bound = 4 * max(e32, 2.0 ** -24 * abs(float(ref64)))
    assert abs(float(out.detach()) - float(parts)) <= 2 * bound
    g64 = _autograd(lr.hierarchy, x, t)(torch.float64)
    assert float((dxg.grad - pgrad).norm()) / float(g64.norm()) <= 2 * 4e-6


def test_determinism():
    x, t = _hier_inputs((2, 1, 97, 130), seed=9)
    dx, dt_ = x.to(_dev()), t.to(_dev())
    for fn in (optics.hierarchy_loss, optics.ssim, optics.dice_loss, optics.bce_with_logits,
               lambda a, b: optics.dice_loss(a, b, p=3)):
        a, ga = _fwd_bwd(fn, dx, dt_)
        b, gb = _fwd_bwd(fn, dx, dt_)
        assert _bits(a, b) and _bits(ga, gb)
    # the sums do not depend on the alignment of the arrays
    a, ga = _fwd_bwd(optics.dice_loss, _place(x, 1), _place(t, 1))
    b, gb = _fwd_bwd(optics.dice_loss, dx, dt_)
    assert _bits(a, b) and _bits(ga, gb)


def test_graph_capture_replays_on_new_contents():
    x, t = _hier_inputs((2, 1, 43, 75), seed=3)
    sx, st = x.to(_dev()).requires_grad_(True), t.to(_dev())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            torch.autograd.grad(optics.hierarchy_loss(sx, st), sx)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s_loss = optics.hierarchy_loss(sx, st)
        s_grad, = torch.autograd.grad(s_loss, sx)
    for seed in (21, 22):
        x2, t2 = _hier_inputs((2, 1, 43, 75), seed=seed)
        with torch.no_grad():
            sx.copy_(x2)
            st.copy_(t2)
        graph.replay()
        torch.cuda.synchronize()
        want, gwant = _fwd_bwd(optics.hierarchy_loss, x2.to(_dev()), t2.to(_dev()))
        assert _bits(s_loss.detach(), want) and _bits(s_grad, gwant)


def test_moderate_size():
    shape = (4, 1, 512, 512)
    x, t = _hier_inputs(shape, seed=13)
    dx, dt_ = x.to(_dev()), t.to(_dev())
    _value("ssim", f"{shape}", optics.ssim(dx, dt_), lambda dt: lr.ssim(x.to(dt), t.to(dt)))
    _value("dice", f"{shape}", optics.dice_loss(dx, dt_), lambda dt: lr.dice(x.to(dt), t.to(dt)))
    _value("bce", f"{shape}", optics.bce_with_logits(dx, dt_), lambda dt: lr.bce(x.to(dt), t.to(dt)))
    out, g = _fwd_bwd(optics.hierarchy_loss, dx, dt_)
    _value("hierarchy", f"{shape}", out, lambda dt: lr.hierarchy(x.to(dt), t.to(dt)))
    _grad("hierarchy", f"{shape}", g, _autograd(lr.hierarchy, x, t))
