"""The height-map kernels on the GPU (thz_heightmap.hip through optics.lut_quantize / center_difference /
total_variation, utils.Helper_Functions and Components.quantization).

Quantizer forward: q and idx are compared bit for bit with torch's own bucketize / argmin on the device
and with the reference's outputs (tests/golden/heightmap_golden.npz).

Everything else is held to tests/heightmap_ref.py in float64 on the CPU (pinned by
tests/test_heightmap_cpu.py):
    |kernel - fp64| <= 4 x max(e32, 2^-24 |value|)
in the maximum norm over a quantity's elements, e32 the error of the float32 op sequence on the same
input (the restatement run in float32; for the Components classes the reference's own float32
outputs of the fixture), the rule of tests/test_losses_gpu.py.  The total-variation gradient, a sum of
at most eight terms +-W / (4 N H W), +-H / (4 N H W), is compared in the relative L2 norm against the float64
autograd of the restatement, <= 4 x max(e32, 2^-24).

Every comparison prints its ratio err / bound; THZ_HEIGHTMAP_PARITY_LOG=<file> writes the largest per
quantity there (profiles/heightmap_parity_ratios.txt is such a run on an MI355X).
"""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from quantizationawarethzdoe_amd import _lib, optics
from quantizationawarethzdoe_amd.Components import quantization as Q
from quantizationawarethzdoe_amd.Components.discrete_doe import DiscreteDOE
from quantizationawarethzdoe_amd.utils import Helper_Functions as HF
from tests import heightmap_ref as hr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "heightmap_golden.npz"))
S = {"1": 1.0, "2p5": 2.5, "11": 11.0}
RATIOS = {}


def _dev():
    return torch.device("cuda:0")


def _g(name):
    return torch.from_numpy(G[name])


@pytest.fixture(scope="module", autouse=True)
def _ratio_log():
    yield
    path = os.environ.get("THZ_HEIGHTMAP_PARITY_LOG")
    if path:
        with open(path, "w") as fh:
            fh.write("# largest err / bound per quantity; bound = 4 max(e32, 2^-24 |value|) in the maximum norm "
                     "(values), 4 max(e32, 2^-24) (total-variation gradient, relative L2)\n")
            for k in sorted(RATIOS):
                fh.write(f"{k:28s} {RATIOS[k][0]:.4f}   ({RATIOS[k][1]})\n")


def _note(what, case, ratio):
    print(f"{what:26s} {case:60s} err / bound = {ratio:.4f}")
    if what not in RATIOS or ratio > RATIOS[what][0]:
        RATIOS[what] = (ratio, case)


def _value(what, case, got, r64, r32):
    got = got.detach().cpu().double()
    assert got.shape == r64.shape, (got.shape, r64.shape)
    assert bool(torch.isfinite(got).all())
    err = float((got - r64).abs().max())
    e32 = float((r32.double() - r64).abs().max())
    bound = 4 * max(e32, 2.0 ** -24 * float(r64.abs().max()))
    _note(what, case, err / bound if bound else float(err > 0))
    assert err <= bound, (what, case, err, e32, bound)


def _bits(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


def _place(t, offset=0):
    """A contiguous device copy whose pointer is 16-byte aligned (offset 0) or one element past."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=_dev())
    v = buf[offset:offset + t.numel()].view(t.shape)
    v.copy_(t)
    assert (v.data_ptr() % 16 == 0) == (offset == 0)
    return v.detach()


# ---- quantizer forward -------------------------------------------------------------------------
def _tables():
    out = {str(t): [float(v) for v in np.float32(G[f"lut_{t}"])] for t in G["tables"]}
    out["one"] = [0.25e-3]
    out["two"] = [0.0, 1e-3]
    return out


TABLES = _tables()


def _mid32(lut):
    return [float((np.float32(a) + np.float32(b)) / np.float32(2)) for a, b in zip(lut[:-1], lut[1:])]


def _edge_inputs(lut, thr, n):
    """n values: every threshold and level, the floats beside every threshold, below and above the
    table, +-0, NaN, then seeded values across and beyond the table."""
    pts = np.float32(list(thr) + list(lut))
    t = np.float32(thr)
    span = max(float(lut[-1] - lut[0]), 1e-3)
    edge = np.concatenate([pts, np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf)),
                           np.float32([lut[0] - span, lut[-1] + span, lut[0] - 1e3, lut[-1] + 1e3, 0.0, -0.0, np.nan])])
    rng = np.random.default_rng(len(lut) * 1000 + n)
    rest = np.float32(rng.uniform(lut[0] - 0.3 * span, lut[-1] + 0.3 * span, max(n, len(edge))))
    x = np.concatenate([edge, rest])[:n] if n >= len(edge) else np.concatenate([edge[:n // 2], rest])[:n]
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))


def _check_forward(x, lut, mode, wrap, thr, offset=0):
    xd = _place(x, offset)
    kw = dict(mode=mode, wrap=wrap, surrogate=None)
    if mode == "bucketize":
        kw["midvals"] = thr
    q, idx = optics.lut_quantize(xd, lut, **kw)
    tq, tidx = optics.heightmap.lut_forward_torch(xd, tuple(lut), tuple(thr), optics.heightmap.LUT_MODES[mode], wrap)
    assert idx.dtype == torch.int64 and not q.requires_grad and q.shape == x.shape
    assert torch.equal(idx, tidx), (mode, wrap, len(lut), x.numel())
    assert _bits(q, tq)
    rq, ridx = hr.quantize(x, lut, thr, mode, wrap)  # the CPU restatement agrees too
    assert torch.equal(idx.cpu(), ridx) and _bits(q, rq)


LENGTHS = [1, 3, 4, 5, 255, 257, 64 * 4 * 9 + 1]


@pytest.mark.parametrize("table", ["one", "two", "u16", "n16", "n9"])
def test_quantize_forward_edges_and_lengths(table):
    lut = TABLES[table]
    thr = _mid32(lut)
    big = _edge_inputs(lut, thr, 64 * 4 * 9 + 1)
    assert bool(torch.isnan(big).any()) and float(big[~torch.isnan(big)].min()) < lut[0] <= lut[-1] < float(
        big[~torch.isnan(big)].max())
    for n in LENGTHS:
        x = big if n == big.numel() else _edge_inputs(lut, thr, n)
        for offset in (0, 1):
            _check_forward(x, lut, "argmin", False, [], offset)
            _check_forward(x, lut, "bucketize", False, thr, offset)
            if thr:
                _check_forward(x, lut, "bucketize", True, thr, offset)
            _check_forward(x, lut, "bucketize", True, thr + [lut[-1] + 1e-4], offset)  # T = L thresholds, wrapped


def test_quantize_forward_nan_and_wrap_rules():
    lut = TABLES["u4"]
    thr = _mid32(lut)
    x = torch.tensor([float("nan"), lut[-1] + 1.0, thr[-1], lut[0] - 1.0, 0.0, -0.0]).to(_dev())
    assert optics.heightmap.lut_forward_torch(x, tuple(lut), tuple(thr), _lib.LUTQ_BUCKETIZE, False)[1].tolist() == [3, 3, 3, 0, 0, 0]
    _, idx = optics.lut_quantize(x, lut, surrogate=None)
    assert idx.tolist() == [3, 3, 3, 0, 0, 0]  # a NaN counts every threshold, as torch.bucketize
    _, idx = optics.lut_quantize(x, lut, wrap=True, surrogate=None)
    assert idx.tolist() == [0, 0, 0, 0, 0, 0]  # the reference's modulo: the top bucket is level 0
    _, idx = optics.lut_quantize(x[[0, 1, 3, 4, 5]], lut, mode="argmin", surrogate=None)
    assert idx.tolist() == [0, 3, 0, 0, 0]  # a NaN distance never wins: index 0, as torch.argmin gives
    tie = torch.tensor([0.5, 1.5, 2.5]).to(_dev())
    _, idx = optics.lut_quantize(tie, [0.0, 1.0, 2.0, 3.0], mode="argmin", surrogate=None)
    assert idx.tolist() == [0, 1, 2]  # ties go to the lower index


@pytest.mark.parametrize("p", ["f32", "f64"])
def test_quantize_forward_matches_the_fixture(p):
    x = _g(f"xq_{p}").to(_dev())
    for t in G["tables"]:
        lut = _g(f"lut_{t}").to(x.dtype)
        q, idx = HF.nearest_neighbor_search(x, lut, _g(f"mid_{t}_{p}"))
        assert torch.equal(idx.cpu(), _g(f"idx_{t}_{p}")) and torch.equal(q.cpu(), _g(f"q_{t}_{p}"))
        assert torch.equal(HF.nearest_idx(x, _g(f"mid_{t}_{p}")).cpu(), _g(f"idx_{t}_{p}"))
    snap = _g(f"snap_x_{p}").to(_dev())
    for k in "123":
        q, idx = optics.lut_quantize(snap, _g(f"snap_lut_{k}").to(snap.dtype), mode="argmin", surrogate=None)
        assert torch.equal(idx.cpu(), _g(f"snap_idx_{k}_{p}")) and torch.equal(q.cpu(), _g(f"snap_q_{k}_{p}"))


def test_device_tables_are_read_afresh_every_call():
    """Same-length device tables created back to back (the allocator hands the freed block straight
    back, at version 0), one updated through .data, one in place: each call quantizes to the values
    the table holds then."""
    x = torch.linspace(-0.1, 1.3, 257).to(_dev())
    addresses = set()
    for h in (1.0, 0.5, 0.25, 2.0):
        lut = torch.linspace(0, h, 8, device=_dev())
        addresses.add(lut.data_ptr())
        want = lut.cpu()
        for mode, fn in (("argmin", lambda: optics.lut_quantize(x, lut, mode="argmin", surrogate=None)),
                         ("bucketize", lambda: optics.lut_quantize(x, lut, wrap=False, surrogate=None)),
                         ("search", lambda: HF.nearest_neighbor_search(x, lut, torch.tensor(HF.lut_mid(lut))))):
            q, idx = fn()
            rq, ridx = hr.quantize(x.cpu(), want, _mid32(want.tolist()), "argmin" if mode == "argmin" else "bucketize",
                                   wrap=mode == "search")
            assert torch.equal(idx.cpu(), ridx) and _bits(q, rq), (h, mode)
        del lut
    lut = torch.linspace(0, 1.0, 8, device=_dev())
    for update in (lambda: lut.data.mul_(0.5), lambda: lut.mul_(3.0)):
        optics.lut_quantize(x, lut, mode="argmin", surrogate=None)
        update()
        q, idx = optics.lut_quantize(x, lut, mode="argmin", surrogate=None)
        rq, ridx = hr.quantize(x.cpu(), lut.cpu(), mode="argmin")
        assert torch.equal(idx.cpu(), ridx) and _bits(q, rq)
    print("distinct table addresses over four tables:", len(addresses))


def test_device_table_is_refused_during_capture():
    x = torch.rand(64, device=_dev())
    lut = torch.linspace(0, 1.0, 8, device=_dev())
    optics.lut_quantize(x, lut, surrogate=None)
    host = lut.cpu()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="list or a CPU tensor"):
            optics.lut_quantize(x, lut, surrogate=None)
        q, _ = optics.lut_quantize(x, host, surrogate=None)  # the CPU table captures
    graph.replay()
    torch.cuda.synchronize()
    assert _bits(q, optics.lut_quantize(x, lut, surrogate=None)[0])


def test_quantize_argument_errors():
    x = torch.zeros(8, device=_dev())
    with pytest.raises(ValueError, match="levels"):
        optics.lut_quantize(x, [0.1 * i for i in range(_lib.THZ_MAX_LUT + 1)])
    with pytest.raises(ValueError, match="levels"):
        HF.nearest_idx(x, [0.1 * i for i in range(_lib.THZ_MAX_LUT + 1)])
    with pytest.raises(ValueError, match="thresholds"):
        optics.lut_quantize(x, [0.0, 1.0], midvals=[0.2, 0.5])
    with pytest.raises(TypeError, match="float32"):
        optics.lut_quantize(x.half(), [0.0, 1.0])
    with pytest.raises(TypeError, match="float32"):
        optics.total_variation(torch.zeros(1, 1, 4, 4, dtype=torch.int32, device=_dev()))
    with pytest.raises(TypeError):
        HF.nearest_neighbor_search(x, [0.0, 1.0])  # no thresholds: the reference's len(None)


# ---- quantizer backward ------------------------------------------------------------------------
def _backward_inputs(lut, thr):
    """Seeded values across and beyond the table, every level itself (x == q), values just inside the
    lowest and beyond the highest level (the wrap-around other end)."""
    span = float(lut[-1] - lut[0])
    rng = np.random.default_rng(5)
    x = np.concatenate([np.float32(lut), np.float32([lut[0] - 0.2 * span, lut[0] - 0.01 * span, lut[-1] + 0.01 * span,
                                                     lut[-1] + 0.3 * span]),
                        np.float32(rng.uniform(lut[0] - 0.1 * span, lut[-1] + 0.1 * span, 1100))])
    return torch.from_numpy(x.astype(np.float32))


@pytest.mark.parametrize("kind", ["identity", "poly", "sigmoid"])
@pytest.mark.parametrize("table,wrap", [("n9", True), ("u4", False), ("n16", True)])
def test_quantize_backward(table, wrap, kind):
    lut = TABLES[table]
    thr = _mid32(lut)
    x = _backward_inputs(lut, thr)
    up = torch.from_numpy(np.random.default_rng(6).standard_normal(x.numel()).astype(np.float32))
    _, idx = hr.quantize(x, lut, thr, wrap=wrap)
    assert int((x == torch.tensor(lut)[idx]).sum()) >= len(lut) - 1 and int(idx.min()) == 0
    for tag, s in S.items():
        for offset in (0, 1):
            xd = _place(x, offset).requires_grad_(True)
            q, gidx = optics.lut_quantize(xd, lut, midvals=thr, wrap=wrap, surrogate=kind, s=s)
            assert torch.equal(gidx.cpu(), idx) and not gidx.requires_grad
            (q * up.to(_dev())).sum().backward()
            r64 = up.double() * hr.slope(x.double(), idx, lut, kind, s)
            r32 = up * hr.slope(x, idx, lut, kind, s)
            _value(f"lut {kind} grad", f"{table} wrap={wrap} s={tag} +{offset}", xd.grad, r64, r32)
    if kind == "poly":  # s = 1: (1 - |z|)^0 = 1 everywhere, 0^0 at the levels included
        xd = x.to(_dev()).requires_grad_(True)
        optics.lut_quantize(xd, lut, midvals=thr, wrap=wrap, surrogate="poly", s=1.0)[0].sum().backward()
        assert torch.equal(xd.grad.cpu(), torch.ones_like(x))


def test_quantize_backward_float64_runs_the_torch_sequence():
    lut, thr = TABLES["n9"], _mid32(TABLES["n9"])
    x = _backward_inputs(lut, thr).double()
    _, idx = hr.quantize(x, lut, thr, wrap=True)
    for kind in ("poly", "sigmoid"):
        xd = x.to(_dev()).requires_grad_(True)
        q, _ = optics.lut_quantize(xd, lut, midvals=thr, wrap=True, surrogate=kind, s=2.5)
        assert q.dtype == torch.float64
        q.sum().backward()
        want = hr.slope(x, idx, lut, kind, 2.5)
        assert float((xd.grad.cpu() - want).abs().max()) <= 1e-9 * float(want.abs().max())


def test_identity_kind_of_the_c_entry():
    g = torch.randn(1027, device=_dev())
    out = torch.empty_like(g)
    d = optics.heightmap.lut_desc(g.numel(), 0, False, _lib.LUTQ_GRAD_IDENTITY, (0.0, 1.0), ())
    _lib.check(_lib.lib().thz_lut_quantize_backward(ctypes.byref(d), None, None, ctypes.c_void_p(g.data_ptr()), None,
                                                    ctypes.c_void_p(out.data_ptr()),
                                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert _bits(out, g)


def test_steepness_is_read_on_the_device_at_replay():
    lut, thr = TABLES["n9"], _mid32(TABLES["n9"])
    x = _backward_inputs(lut, thr)
    _, idx = hr.quantize(x, lut, thr, wrap=True)
    sx = x.to(_dev()).requires_grad_(True)
    s = torch.tensor(2.5, device=_dev())

    def step():
        q, _ = optics.lut_quantize(sx, lut, midvals=thr, wrap=True, surrogate="sigmoid", s=s)
        return torch.autograd.grad(q.sum(), sx)[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        grad = step()
    for value in (1.0, 7.0):
        s.fill_(value)
        graph.replay()
        torch.cuda.synchronize()
        r64 = hr.slope(x.double(), idx, lut, "sigmoid", value)
        _value("lut sigmoid grad", f"graph replay s={value}", grad, r64, hr.slope(x, idx, lut, "sigmoid", value))


# ---- center_difference / total_variation --------------------------------------------------------
TV_SHAPES = [(1, 1, 1, 1), (1, 1, 2, 2), (1, 1, 1, 7), (1, 1, 3, 3), (2, 3, 37, 53), (1, 2, 130, 257),
             (1, 2, 1, 2, 9, 11), (1, 1, 40, 64)]


def _tv_input(shape):
    if shape == (2, 3, 37, 53):
        return _g("tv_x4_f32")
    if shape == (1, 2, 1, 2, 9, 11):
        return _g("tv_x6_f32")
    return torch.randn(shape, generator=torch.Generator().manual_seed(sum(shape)))


def _rel_l2(what, case, got, g64, g32):
    got = got.detach().cpu().double()
    assert got.shape == g64.shape and bool(torch.isfinite(got).all())
    nrm = float(g64.norm())
    if nrm == 0:
        assert float(got.abs().max()) == 0
        return
    err, e32 = float((got - g64).norm()) / nrm, float((g32.double() - g64).norm()) / nrm
    bound = 4 * max(e32, 2.0 ** -24)
    _note(what, case, err / bound)
    assert err <= bound, (what, case, err, e32, bound)


def _tv_grad(x, dtype):
    xa = x.detach().to(dtype).clone().requires_grad_(True)
    hr.total_variation(xa).backward()
    return xa.grad


@pytest.mark.parametrize("shape", TV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_center_difference_and_total_variation(shape):
    x = _tv_input(shape)
    for offset in (0, 1):
        xd = _place(x, offset).requires_grad_(True)
        dx, dy = optics.center_difference(xd)
        r64, r32 = hr.center_difference(x.double()), hr.center_difference(x)
        _value("center_difference dx", f"{shape} +{offset}", dx, r64[0], r32[0])
        _value("center_difference dy", f"{shape} +{offset}", dy, r64[1], r32[1])
        tv = optics.total_variation(xd)
        assert tv.shape == () and tv.dtype == torch.float32
        _value("total_variation", f"{shape} +{offset}", tv, hr.total_variation(x.double()), hr.total_variation(x))
        assert _bits(tv, optics.total_variation(xd))  # a fixed summation order
        # interior values of a random input are never exactly zero, so the sign is the float64 one
        dz = torch.cat([r64[0][..., 1:-1].reshape(-1), r64[1][..., 1:-1, :].reshape(-1)])
        assert dz.numel() == 0 or float(dz.abs().min()) > 0
        tv.backward()
        _rel_l2("total_variation grad", f"{shape} +{offset}", xd.grad, _tv_grad(x, torch.float64),
                _tv_grad(x, torch.float32))
    if len(shape) == 6:  # the reference-named helper views [B T P, C, H, W]
        assert _bits(HF.total_variation(x.to(_dev())), tv)
        assert torch.equal(dx.cpu().reshape(G["cd_dx_x6_f32"].shape), HF.center_difference(
            x.to(_dev()).view(-1, *shape[-3:]))[0].cpu())
    if shape == (2, 3, 37, 53):  # the reference's own float32 outputs bound the kernel the same way
        _value("center_difference dx", "fixture", dx, _g("cd_dx_x4_f64"), _g("cd_dx_x4_f32"))
        _value("total_variation", "fixture", tv, _g("tvval_x4_f64"), _g("tvval_x4_f32"))


def test_tv_non_contiguous_and_float64():
    x = _tv_input((2, 3, 37, 53))
    xt = x.to(_dev()).transpose(-1, -2)
    assert not xt.is_contiguous()
    xt = xt.requires_grad_(True)
    tv = optics.total_variation(xt)
    ref = x.transpose(-1, -2).contiguous()
    _value("total_variation", "transposed view", tv, hr.total_variation(ref.double()), hr.total_variation(ref))
    tv.backward()
    _rel_l2("total_variation grad", "transposed view", xt.grad, _tv_grad(ref, torch.float64), _tv_grad(ref, torch.float32))
    x64 = x.double().to(_dev()).requires_grad_(True)
    tv64 = optics.total_variation(x64)
    assert tv64.dtype == torch.float64 and abs(float(tv64.detach()) - float(_g("tvval_x4_f64"))) <= 1e-12 * float(tv64.detach())
    tv64.backward()
    assert float((x64.grad.cpu() - _g("tv_grad_x4_f64")).abs().max()) <= 1e-15
    dx64, _ = optics.center_difference(x64)
    assert float((dx64.detach().cpu() - _g("cd_dx_x4_f64")).abs().max()) <= 1e-12


def test_tv_gradient_takes_sign_zero_as_zero():
    """Integer-valued maps: many second differences are exactly zero in any precision, and there the
    gradient takes sign(0) = 0, as torch's abs backward."""
    g = torch.Generator().manual_seed(17)
    x = torch.randint(-2, 3, (1, 2, 35, 70), generator=g).float()
    r64 = hr.center_difference(x.double())
    assert int((r64[0][..., 1:-1] == 0).sum()) > 100 and int((r64[1][..., 1:-1, :] == 0).sum()) > 100
    xd = x.to(_dev()).requires_grad_(True)
    (3 * optics.total_variation(xd)).backward()
    want = 3 * _tv_grad(x, torch.float64)
    _rel_l2("total_variation grad", "integer map, sign(0)", xd.grad, want, 3 * _tv_grad(x, torch.float32))
    flat = torch.full((1, 1, 9, 260), 0.37, device=_dev(), requires_grad=True)
    optics.total_variation(flat).backward()
    assert float(flat.grad.abs().max()) == 0


@pytest.mark.parametrize("shape", [(1, 1, 3, 3), (2, 3, 37, 53), (1, 2, 130, 257), (1, 1, 40, 64), (1, 1, 1, 7)],
                         ids=lambda s: "x".join(map(str, s)))
def test_center_difference_backward(shape):
    x = _tv_input(shape)
    g = torch.Generator().manual_seed(23)
    cx, cy = torch.randn(shape, generator=g), torch.randn(shape, generator=g)

    def ref(dtype):
        xa = x.to(dtype).clone().requires_grad_(True)
        dx, dy = hr.center_difference(xa)
        ((dx * cx.to(dtype)).sum() + (dy * cy.to(dtype)).sum()).backward()
        return xa.grad

    xd = x.to(_dev()).requires_grad_(True)
    dx, dy = optics.center_difference(xd)
    ((dx * cx.to(_dev())).sum() + (dy * cy.to(_dev())).sum()).backward()
    _value("center_difference grad", f"{shape}", xd.grad, ref(torch.float64), ref(torch.float32))


# ---- capture, Components -------------------------------------------------------------------------
def test_regulariser_and_quantizer_capture_in_one_graph():
    """total_variation(x) + lut_quantize(x)[0].sum(), forward and backward, captured: a host sync inside
    either would fail the capture; the replay on new contents equals the eager result bit for bit."""
    lut = [v * 1e3 for v in TABLES["n9"]]
    shape = (2, 1, 37, 53)
    sx = torch.rand(shape, device=_dev()).requires_grad_(True)
    s = torch.tensor(3.0, device=_dev())

    def step(x):
        loss = optics.total_variation(x) + optics.lut_quantize(x, lut, wrap=True, midvals=_mid32(lut),
                                                               surrogate="poly", s=s)[0].sum()
        return loss, torch.autograd.grad(loss, x)[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step(sx)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s_loss, s_grad = step(sx)
    for seed in (31, 32):
        x2 = torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 1.2 - 0.1
        with torch.no_grad():
            sx.copy_(x2)
        graph.replay()
        torch.cuda.synchronize()
        want, gwant = step(x2.to(_dev()).requires_grad_(True))
        assert _bits(s_loss.detach(), want.detach()) and _bits(s_grad, gwant)


@pytest.fixture
def class_table():
    """DiscreteDOE.lut / lut_midvals assigned on the class, as a user of the reference does; restored."""
    saved = {k: DiscreteDOE.__dict__[k] for k in ("lut", "lut_midvals")}
    lut = _g("lut_n9").float()
    DiscreteDOE.lut = lut.to(_dev())
    DiscreteDOE.lut_midvals = torch.tensor(HF.lut_mid(lut))
    assert torch.equal(DiscreteDOE.lut_midvals, _g("mid_n9_f32"))
    yield lut
    for k, v in saved.items():
        setattr(DiscreteDOE, k, v)


def test_components_quantizers_reproduce_the_fixture(class_table):
    x, up = _g("nns_x_f32"), _g("nns_g_f32")
    fns = {"identity": (Q.nns, Q.NearestNeighborSearch), "poly": (Q.nns_poly, Q.NearestNeighborPolyGrad),
           "sigmoid": (Q.nns_sigmoid, Q.NearestNeighborSigmoidGrad)}
    for kind, (fn, cls) in fns.items():
        for tag, s in S.items():
            xd = x.to(_dev()).requires_grad_(True)
            q = fn(xd, torch.tensor(s))
            assert _bits(q, _g("nns_q_f32")) and _bits(cls.apply(xd, torch.tensor(s, device=_dev())), q)
            q.backward(up.to(_dev()))
            _value(f"nns {kind} grad", f"fixture s={tag}", xd.grad, _g(f"nns_grad_{kind}_{tag}_f64"),
                   _g(f"nns_grad_{kind}_{tag}_f32"))
    qz = Q.Quantization("nn_sigmoid", lut=[float(v) for v in class_table], num_bits=3, dev=_dev())
    xd = x.to(_dev()).requires_grad_(True)
    out = qz(xd, float(G["quant_iter_frac"]))
    assert _bits(out, _g("quant_sigmoid_f32"))
    out.sum().backward()
    s = 1 + 10 * float(G["quant_iter_frac"])
    _, idx = hr.quantize(x, class_table, _g("mid_n9_f32"), wrap=True)
    _value("nns sigmoid grad", "Quantization('nn_sigmoid')", xd.grad, hr.slope(x.double(), idx, class_table.double(), "sigmoid", s),
           _g("quant_sigmoid_grad_f32"))
    assert Q.Quantization("nn", lut=[float(v) for v in class_table], num_bits=3, dev=_dev())(xd, 0.5).shape == (13, 17)


def test_softmax_quantizer_runs_the_torch_sequence():
    lut = torch.linspace(0, 1e-3, 9)
    torch.manual_seed(0)
    x = (torch.rand(1, 1, 12, 10) * 1e-3).to(_dev()).requires_grad_(True)
    soft = Q.Quantization("softmax", lut=lut.tolist(), num_bits=3, dev=_dev())
    out = soft(x, 1.0, hard=True)
    snapped = optics.lut_quantize(x, lut[:-1], mode="argmin", surrogate=None)[0]
    assert out.shape == (12, 10) and float((out.detach() - snapped[0, 0]).abs().max()) <= 1e-8
    with pytest.raises(RuntimeError, match="inplace"):  # score_thickness normalises in place, as the reference does
        out.sum().backward()
    gum = Q.Quantization("gumbel_softmax", lut=lut.tolist(), num_bits=3, dev=_dev())(x, 0.5)
    assert gum.shape == (12, 10) and math.isfinite(float(gum.detach().sum()))
