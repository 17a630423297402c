"""The cases of tests/test_stream_bits_gpu.py and tests/golden/gen_stream_bits.py: the public entries that
run on the streaming toolkit (csrc/thz_stream.hpp), on seeded inputs whose shapes reach every branch of it.

    a      one partial with a ragged tail (1027 elements, a 33 x 31 plane): the bound-checked group
    wide   the same kind of data at a multiple of four (1028, 32 x 32): the 16-byte form
    b      the data of ``a`` one element past 16-byte alignment: the element-width form; where both exist
           the result must equal ``a`` bit for bit (PAIRS)
    c      more partials per item than the finish workgroup has threads (256): the gather loop's second stride
    d      signal_scale above 1024 x 1024 floats: the producers' grid-stride loop wraps

``run_case(name)`` returns {output name: integer bit view on the CPU}; an output of more than DIGEST_ABOVE
values is returned as the SHA-256 of its bytes (uint8 [32]) under "<output>#sha256", which keeps the fixture
small and still compares every bit.  Each case seeds its own generator, so a case's inputs do not depend on
which other cases ran.
"""
import hashlib
import zlib

import numpy as np
import torch

from quantizationawarethzdoe_amd import optics

SEED = 20261021
DIGEST_ABOVE = 4096


def _rng(name):
    return np.random.default_rng([SEED, zlib.crc32(name.encode())])


def _place(a, device, off):
    """The array on the device, contiguous; off: its first element one element past 16-byte alignment."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not off:
        return t.to(device)
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=device)
    assert buf.data_ptr() % 16 == 0
    buf[1:].copy_(t.reshape(-1))
    v = buf[1:].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def bits(t):
    """The integer view of a tensor's bits, on the CPU."""
    t = t.detach()
    if t.is_complex():
        t = torch.view_as_real(t.resolve_conj())
    t = t.contiguous()
    if t.dtype == torch.float32:
        t = t.view(torch.int32)
    elif t.dtype == torch.float64:
        t = t.view(torch.int64)
    elif t.dtype == torch.bool:
        t = t.to(torch.uint8)
    return t.cpu()


def _f32(r, shape, lo=-1.0, hi=1.0):
    return r.uniform(lo, hi, size=shape).astype(np.float32)


def _c64(r, shape):
    return (r.standard_normal(shape) + 1j * r.standard_normal(shape)).astype(np.complex64)


# ---- the entries -----------------------------------------------------------------------------------
def _signal_scale(name, device, n, cplx=False, off=False):
    r = _rng(name)
    x = _place(_c64(r, n) if cplx else _f32(r, n), device, off)
    return {"scale": optics.signal_scale(x, 7.5)}


def _snr_noise(name, device, n, cplx=False, off=False):
    r = _rng(name)
    x = _place(_c64(r, n) if cplx else _f32(r, n), device, off).requires_grad_()
    g = _place(_c64(r, n) if cplx else _f32(r, n), device, off)
    state = torch.tensor([12345, 7], dtype=torch.int32, device=device)
    y = optics.add_noise(x, "gauss", snr_db=12.0, rng=(state, 3))
    (gx,) = torch.autograd.grad(y, x, g)
    return {"y": y, "gx": gx}


def _dice(name, device, N, M, p=2, off=False):
    r = _rng(name)
    pred = _place(_f32(r, (N, M), 0.0, 1.0), device, off).requires_grad_()
    target = _place((r.uniform(size=(N, M)) < 0.4).astype(np.float32), device, off)
    w = torch.from_numpy(_f32(r, N, 0.5, 1.5)).to(device)
    loss = optics.dice_loss(pred, target, smooth=1, p=p, reduction="none")
    (grad,) = torch.autograd.grad(loss, pred, w)
    return {"loss": loss, "grad": grad}


def _bce(name, device, N, M, weighted=False, reduction="mean", off=False):
    r = _rng(name)
    pred = _place(_f32(r, (N, M), -4.0, 4.0), device, off).requires_grad_()
    target = _place((r.uniform(size=(N, M)) < 0.4).astype(np.float32), device, off)
    kw = {}
    if weighted:
        kw = {"weight": torch.from_numpy(_f32(r, (N, M), 0.5, 1.5)).to(device),
              "pos_weight": torch.from_numpy(_f32(r, M, 0.5, 2.0)).to(device)}
    loss = optics.bce_with_logits(pred, target, reduction=reduction, **kw)
    g = torch.from_numpy(_f32(r, tuple(loss.shape))).to(device)
    (grad,) = torch.autograd.grad(loss, pred, g)
    return {"loss": loss, "grad": grad}


def _ssim(name, device, shape, off=False):
    r = _rng(name)
    xa = _f32(r, shape, 0.0, 1.0)
    x = _place(xa, device, off).requires_grad_()
    y = _place(np.clip(xa + _f32(r, shape, -0.2, 0.2), 0.0, 1.0), device, off)
    v = optics.ssim(x, y, size_average=False)
    g = torch.from_numpy(_f32(r, tuple(v.shape))).to(device)
    (grad,) = torch.autograd.grad(v, x, g)
    return {"ssim": v, "grad": grad}


def _tv(name, device, shape, off=False):
    r = _rng(name)
    x = _place(_f32(r, shape), device, off).requires_grad_()
    tv = optics.total_variation(x)
    (grad,) = torch.autograd.grad(tv, x)
    return {"tv": tv, "grad": grad}


def _regions(H, W):
    # a circle inside the plane, one that leaves it, and a rectangle over most of its rows
    return [[0.4 * H, 0.5 * W, 0.3 * min(H, W), 0.0], [0.9 * H, 0.1 * W, 0.25 * W, 0.0], [0.5 * H, 0.5 * W, 0.4 * H, 0.3 * W]]


def _region_stats(name, device, shape, K, cplx, off=False):
    r = _rng(name)
    x = _place(_c64(r, shape) if cplx else _f32(r, shape, 0.0, 1.0), device, off).requires_grad_()
    H, W = shape[-2:]
    st = optics.region_stats(x, _regions(H, W)[:K], ["circ", "circ", "rect"][:K])
    gp = torch.from_numpy(r.uniform(-1.0, 1.0, size=tuple(st.power.shape))).to(device)
    g1 = torch.from_numpy(r.uniform(-1.0, 1.0, size=tuple(st.moment1.shape)) / max(H, W)).to(device)
    g2 = torch.from_numpy(r.uniform(-1.0, 1.0, size=tuple(st.moment2.shape)) / max(H, W) ** 2).to(device)
    (grad,) = torch.autograd.grad((st.power, st.moment1, st.moment2), x, (gp, g1, g2))
    return {"power": st.power, "moment1": st.moment1, "moment2": st.moment2, "peak": st.peak, "argmax": st.argmax,
            "count": st.count, "grad": grad}


def _ifta(name, device, shape, masked, off=False):
    r = _rng(name)
    N, H, W = shape
    U = _place(_c64(r, shape), device, off)
    T = _place(_f32(r, (H, W), 0.0, 1.0), device, off)
    mask = None
    if masked:
        ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        mask = torch.from_numpy((ii - 0.5 * H) ** 2 + (jj - 0.4 * W) ** 2 <= (0.35 * min(H, W)) ** 2).to(device)
    stats = optics.ifta_target_stats(U, T, mask)
    out = optics.ifta_target_project(U, T, stats[:, 4], mask, alpha=1.3, beta=0.5)
    return {"stats": stats, "projected": out}


LUT = [0.0, 0.1, 0.25, 0.3, 0.55, 0.6, 0.8, 1.0]


def _lut(name, device, n, mode, surrogate, off=False):
    r = _rng(name)
    x = _place(_f32(r, n, -0.1, 1.1), device, off).requires_grad_()
    g = _place(_f32(r, n), device, off)
    q, idx = optics.lut_quantize(x, LUT, mode=mode, surrogate=surrogate, s=2.5)
    (grad,) = torch.autograd.grad(q, x, g)
    return {"q": q, "idx": idx, "grad": grad}


def _stokes(name, device, shape, off=False):
    r = _rng(name)
    x = _place(_c64(r, shape), device, off).requires_grad_()
    s = optics.stokes(x)
    g = torch.from_numpy(_f32(r, tuple(s.shape))).to(device)
    (grad,) = torch.autograd.grad(s, x, g)
    return {"stokes": s, "grad": grad}


# name -> (function, keyword arguments).  The seed of a case is its name without the ".b" suffix, so a case
# and its misaligned twin see the same values.
CASES = {}


def _add(name, fn, twin=False, **kw):
    CASES[name] = (fn, name, kw)
    if twin:
        CASES[name + ".b"] = (fn, name, dict(kw, off=True))


_add("signal_scale.a", _signal_scale, True, n=1027)
_add("signal_scale.wide", _signal_scale, True, n=1028)
_add("signal_scale.cplx", _signal_scale, True, n=515, cplx=True)
_add("signal_scale.c", _signal_scale, n=1024 * 300 + 5)
_add("signal_scale.d", _signal_scale, n=1024 * 1024 + 4099)
_add("snr_noise.a", _snr_noise, True, n=1027)
_add("snr_noise.wide", _snr_noise, True, n=1028)
_add("snr_noise.cplx", _snr_noise, True, n=1027, cplx=True)
_add("snr_noise.c", _snr_noise, n=1024 * 300 + 5)
_add("dice.a", _dice, True, N=3, M=1027)
_add("dice.wide", _dice, True, N=3, M=1028)
_add("dice.p1", _dice, N=3, M=1027, p=1)
_add("dice.p15", _dice, N=3, M=1027, p=1.5)
_add("dice.c", _dice, N=2, M=1024 * 600 + 3)
_add("bce.a", _bce, True, N=3, M=1027)
_add("bce.wide", _bce, True, N=3, M=1028)
_add("bce.weighted", _bce, True, N=3, M=1027, weighted=True)
_add("bce.map", _bce, N=3, M=1027, reduction="none")
_add("ssim.a", _ssim, True, shape=(2, 1, 33, 31))
_add("ssim.c", _ssim, shape=(1, 1, 530, 530))  # 17 x 17 = 289 tiles of 32 x 32 window positions
_add("tv.a", _tv, True, shape=(2, 33, 31))
_add("tv.wide", _tv, True, shape=(2, 33, 32))
_add("tv.c", _tv, shape=(515, 33, 31))  # 1030 tiles of 256 x 32, four per workgroup: 258 partials
for _k in (0, 3):
    for _c in (True, False):
        _t = f"region_stats.K{_k}.{'c64' if _c else 'f32'}"
        _add(_t + ".a", _region_stats, True, shape=(2, 33, 31), K=_k, cplx=_c)
        _add(_t + ".wide", _region_stats, True, shape=(2, 33, 32), K=_k, cplx=_c)
        _add(_t + ".c", _region_stats, shape=(1, 32 * 257 + 5, 31), K=_k, cplx=_c)  # 258 tiles of 256 x 32
for _m in (False, True):
    _t = f"ifta.{'mask' if _m else 'nomask'}"
    _add(_t + ".a", _ifta, True, shape=(2, 33, 31), masked=_m)
    _add(_t + ".wide", _ifta, True, shape=(1, 32, 32), masked=_m)
    _add(_t + ".c", _ifta, shape=(1, 1100, 1000), masked=_m)  # 269 chunks of 4096
_add("lut.bucketize", _lut, True, n=1027, mode="bucketize", surrogate="identity")
_add("lut.bucketize.wide", _lut, True, n=1028, mode="bucketize", surrogate="poly")
_add("lut.argmin", _lut, True, n=1027, mode="argmin", surrogate="sigmoid")
_add("stokes.a", _stokes, True, shape=(3, 33, 31))
_add("stokes.wide", _stokes, True, shape=(3, 32, 32))

# (aligned case, its twin): equal bit for bit -- the 16-byte and the element-width form of a kernel move the
# same values into the same lanes, and the units compile with contraction off
PAIRS = [(n[:-2], n) for n in CASES if n.endswith(".b")]


def run_case(name, device="cuda"):
    fn, seed_name, kw = CASES[name]
    out = {}
    for k, v in fn(seed_name, device, **kw).items():
        v = bits(v)
        if v.numel() > DIGEST_ABOVE:
            k, v = k + "#sha256", torch.frombuffer(bytearray(hashlib.sha256(v.numpy().tobytes()).digest()), dtype=torch.uint8)
        out[k] = v
    return out
