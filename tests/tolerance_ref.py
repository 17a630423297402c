"""The fabrication-tolerance model (include/thzdoe.h: thz_tolerance_*) restated without the kernels.

* ``rng_bits``: the counter-based generator of csrc/thz_dev.hpp in exact uint64 arithmetic (numpy), the 24-bit
  uniforms built on it (exact in float32) and Box-Muller normals in float64 (approximate: the device evaluates log,
  sqrt and cos in float32 -- for statistics only).
* ``heights``: h_k = min(max(((1 + g_k) h + e_{k,l}) + r_k, lo), hi) in float32, one rounding per operation in the
  header's order, on GIVEN standard draws.
* ``screen``: out[k, c] = field[b, c] t_c(h_k[src]) in torch, in the precision of its inputs (fp64 / complex128 as
  the reference, float32 / complex64 as the floor of the parity rule), differentiable by autograd.
"""
import math

import numpy as np
import torch

TAG_SCALE, TAG_LEVEL, TAG_ROUGH = 0x5343414C, 0x4C45564C, 0x524F5547  # "SCAL", "LEVL", "ROUG"
BASE_PLANE = 2e-3
_M32 = 0xFFFFFFFF


def rng_bits(seed, step, stream, idx):
    """rng_bits(rng = (seed, step), stream, idx) of thz_dev.hpp for an array of 32-bit indices, as uint64."""
    idx = np.asarray(idx, dtype=np.uint64)
    hi = ((int(seed) & _M32) ^ ((int(stream) & _M32) * 0x9E3779B9 & _M32)) & _M32
    with np.errstate(over="ignore"):
        x = np.uint64((hi << 32) | (int(step) & _M32)) ^ (idx * np.uint64(0xD1B54A32D192ED03))
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def u01(seed, step, stream, idx):
    """rng_u01: the top 24 bits over 2^24, exact in float32."""
    return (rng_bits(seed, step, stream, idx) >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


def normal64(seed, step, stream, idx):
    """rng_normal in float64: sqrt(-2 log u1) cos(2 pi u2), u1 = (b1 + 1) / 2^24, u2 = b2 / 2^24."""
    w = rng_bits(seed, step, stream, idx)
    u1 = ((w >> np.uint64(40)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = ((w >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


# The fixed case of the statistical GPU test, vetted by tests/test_tolerance_cpu.py on the float64 restatement.
STAT = dict(seed=20261021, step=3, stream=5, K=4096, sigma_scale=0.02, sigma_level=(1e-5, 2e-5, 3e-5, 4e-5),
            a=float(np.float32(5e-6)),  # the float32 the kernel multiplies by: the range check is exact
            pixels=16)


def stat_checks(g, e, r, case=STAT):
    """name -> (|value|, bound) for the scale errors g [K], the level errors e [K, L] and the uniform roughness r
    [K, pixels] (float64 arrays): sample means within 5 sigma / sqrt(K) of 0, sample stds within 5 sigma / sqrt(2 K)
    of sigma, correlations of g with each e_l and of every two levels below 5 / sqrt(K), the roughness inside
    [-a, a) with its mean within 5 a / sqrt(3 pixels K) (a / sqrt(3) is the std of U(-a, a))."""
    K = len(g)
    out = {}
    cols = [("g", g, case["sigma_scale"])] + [(f"e{l}", e[:, l], s) for l, s in enumerate(case["sigma_level"])]
    for name, x, s in cols:
        out[name + ".mean"] = (abs(x.mean()), 5 * s / math.sqrt(K))
        out[name + ".std"] = (abs(x.std() - s), 5 * s / math.sqrt(2 * K))
    for i in range(len(cols)):
        for j in range(i + 1, len(cols)):
            out[f"corr({cols[i][0]},{cols[j][0]})"] = (abs(np.corrcoef(cols[i][1], cols[j][1])[0, 1]), 5 / math.sqrt(K))
    a = case["a"]
    out["r.range"] = (max(r.max() - np.nextafter(a, 0), -a - r.min(), 0.0), 0.0)
    out["r.mean"] = (abs(r.mean()), 5 * a / math.sqrt(3 * r.size))
    return out


def stat_failures(checks):
    return {k: v for k, v in checks.items() if not v[0] <= v[1]}


def nearest_src(out, inp):
    """doe_nearest_src for every destination 0 .. out - 1: float32 scale, floor, clamp."""
    if inp == out:
        return np.arange(out)
    scale = np.float32(inp) / np.float32(out)
    return np.minimum(np.floor(np.arange(out, dtype=np.float32) * scale).astype(np.int64), inp - 1)


def heights(h, idx, sigma_scale, sigma_level, rough, lo, hi, n_scale, n_level, d_rough):
    """[K, hs, ws] float32.  h [hs, ws] float32; idx [hs, ws] int or None; sigma_level a list of L floats; rough =
    None, ("uniform", a) or ("normal", s); n_scale [K] and n_level [K, 16] standard normals, d_rough [K, hs, ws]
    uniforms or normals (float32, the draws the kernel makes).  A zero sigma contributes +0."""
    f = np.float32
    h = np.asarray(h, dtype=f)
    K = len(n_scale)
    g = f(sigma_scale) * np.asarray(n_scale, dtype=f) if sigma_scale != 0.0 else np.zeros(K, dtype=f)
    u = (f(1.0) + g)[:, None, None] * h[None]
    e = np.zeros((K,) + h.shape, dtype=f)
    L = len(sigma_level)
    if idx is not None:
        idx = np.asarray(idx)
        for l in range(L):
            if sigma_level[l] != 0.0:
                el = f(sigma_level[l]) * np.asarray(n_level, dtype=f)[:, l]
                e = np.where((idx == l)[None], el[:, None, None], e)
    u = u + e
    r = np.zeros_like(u)
    if rough is not None and rough[1] != 0.0:
        d = np.asarray(d_rough, dtype=f)
        r = ((d - f(0.5)) * f(2.0)) * f(rough[1]) if rough[0] == "uniform" else f(rough[1]) * d
    u = u + r
    return np.minimum(np.maximum(u, f(lo)), f(hi)).astype(f)


def heights_torch(h, idx, sigma_scale, sigma_level, rough, lo, hi, n_scale, n_level, d_rough):
    """``heights`` in torch, in h's precision, differentiable in h (torch.clamp passes the gradient on [lo, hi])."""
    dt = h.dtype
    g = sigma_scale * n_scale.to(dt)
    u = (1.0 + g)[:, None, None] * h[None]
    if idx is not None:
        table = torch.zeros(n_level.shape[0], 17, dtype=dt)
        for l, s in enumerate(sigma_level):
            table[:, l] = s * n_level[:, l].to(dt)
        safe = torch.where((idx >= 0) & (idx < len(sigma_level)), idx, torch.full_like(idx, 16)).long()
        u = u + table[:, safe.reshape(-1)].reshape(u.shape)
    if rough is not None and rough[1] != 0.0:
        d = d_rough.to(dt)
        u = u + (((d - 0.5) * 2) * rough[1] if rough[0] == "uniform" else rough[1] * d)
    return torch.clamp(u, min=lo, max=hi)


def transmission(h, lam, eps, tand):
    """t(h) of Components/QuantizedDOE.py:47-79 in h's precision."""
    k = 2 * math.pi / lam
    hb = h + BASE_PLANE
    se = math.sqrt(eps)
    return torch.polar(torch.exp(-0.5 * k * hb * tand * se), -k * hb * (se - 1.0))


def screen(field, hk, wavelengths, eps, tand):
    """out [K, C, H, W] = field[b, c] t_c(h_k[src]); field [1 or K, C, H, W], hk [K, hs, ws]."""
    H, W = field.shape[-2:]
    sy = torch.from_numpy(nearest_src(H, hk.shape[-2]))
    sx = torch.from_numpy(nearest_src(W, hk.shape[-1]))
    up = hk[:, sy][:, :, sx]
    t = torch.stack([transmission(up, lam, eps, tand) for lam in wavelengths], dim=1)
    return field * t
