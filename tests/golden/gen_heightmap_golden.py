"""Fixture of the height-map helpers: the reference's own functions on seeded CPU inputs.

Run once, on the CPU, where the reference tree is present:

    python tests/golden/gen_heightmap_golden.py

Writes tests/golden/heightmap_golden.npz.  <p> is f32 or f64, the precision the reference ran in:
  tables                      names of the level tables: u4 u8 u9 u16 (uniform), n4 n8 n9 n16 (non-uniform)
  lut_<t>, mid_<t>_<p>        the levels (float64; exact in float32) and lut_mid of them as torch.tensor makes it
  xq_<p> [257]                inputs from below the lowest to above the highest level
  idx_<t>_<p>, q_<t>_<p>      nearest_idx and nearest_neighbor_search of xq (utils/Helper_Functions.py:375-398)
  nns_x_<p> [1, 1, 13, 17], nns_g_<p>   input and upstream gradient of the quantizers, on table n9
  nns_q_<p>                   nns(x) = nns_poly(x, s) = nns_sigmoid(x, s)
  nns_grad_<kind>_<s>_<p>     the input gradient of nns / nns_poly / nns_sigmoid (kind identity, poly, sigmoid)
                              at s in S (tags 1, 2p5, 11) (Components/quantization.py:59-127)
  quant_sigmoid_<p>, quant_iter_frac   Quantization('nn_sigmoid', lut=n9, num_bits=3)(nns_x, iter_frac) and
                              the gradient of its sum, quant_sigmoid_grad_<p>
  tv_x4_<p> [2, 3, 37, 53], tv_x6_<p> [1, 2, 1, 2, 9, 11]   inputs
  cd_dx_<n>_<p>, cd_dy_<n>_<p>   center_difference (x4; x6 viewed [B T P, C, H, W])   (:56-70)
  tvval_<n>_<p>, tv_grad_<n>_<p> total_variation and its autograd gradient, n in x4, x6 (:40-54)
  snap_x_<p> [1, 1, 33, 29], snap_lut_<k>, snap_q_<k>_<p>, snap_idx_<k>_<p>   the argmin snap of the notebooks'
                              closing cells with their lut_1, lut_2, lut_3 (4, 8, 10 levels of 1 mm).  A notebook
                              cell cannot be imported, so these entries are NOT the reference's output: they come
                              from the cell's formula, argmin_j |input - lut[j]| over a trailing table axis and
                              lut[idx], evaluated by a line of this generator, and pin torch.argmin's result
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _refimport import import_reference  # noqa: E402

S = {"1": 1.0, "2p5": 2.5, "11": 11.0}
ITER_FRAC = 0.3
MM = 1e-3


def tables():
    out = {}
    for n in (4, 8, 9, 16):
        out[f"u{n}"] = (torch.arange(n, dtype=torch.float32) * (MM / n)).double()
        g = torch.Generator().manual_seed(100 + n)
        steps = torch.rand(n, generator=g) + 0.25
        out[f"n{n}"] = ((torch.cumsum(steps, 0) - steps[0]) * (MM / n)).float().double()
    return out


def main():
    ref = import_reference()
    HF = ref.import_module("utils.Helper_Functions")
    Q = ref.import_module("Components.quantization")
    D = ref.import_module("Components.discrete_doe").DiscreteDOE
    out = {}
    tabs = tables()
    out["tables"] = np.array(list(tabs), dtype="U8")
    g = torch.Generator().manual_seed(7)
    xq = (torch.rand(257, generator=g) * 1.5 - 0.25) * MM
    nns_x = torch.rand(1, 1, 13, 17, generator=g) * 1.4 * MM - 0.2 * MM
    nns_g = torch.randn(1, 1, 13, 17, generator=g)
    x4 = torch.randn(2, 3, 37, 53, generator=g)
    x6 = torch.randn(1, 2, 1, 2, 9, 11, generator=g)
    snap_x = torch.rand(1, 1, 33, 29, generator=g) * 1.2 * MM - 0.1 * MM
    for p, dt in (("f32", torch.float32), ("f64", torch.float64)):
        out[f"xq_{p}"] = xq.to(dt).numpy()
        for name, lut64 in tabs.items():
            lut = lut64.to(dt)
            out[f"lut_{name}"] = lut64.numpy()
            mid = torch.tensor(HF.lut_mid(lut))
            assert mid.dtype == dt
            out[f"mid_{name}_{p}"] = mid.numpy()
            out[f"idx_{name}_{p}"] = HF.nearest_idx(xq.to(dt), mid).numpy()
            q, idx = HF.nearest_neighbor_search(xq.to(dt), lut, mid)
            assert np.array_equal(idx.numpy(), out[f"idx_{name}_{p}"])
            out[f"q_{name}_{p}"] = q.numpy()
        # the quantizers read the table from the class (Components/quantization.py:64-65)
        lut = tabs["n9"].to(dt)
        D.lut, D.lut_midvals = lut, torch.tensor(HF.lut_mid(lut))
        x, up = nns_x.to(dt), nns_g.to(dt)
        out[f"nns_x_{p}"], out[f"nns_g_{p}"] = x.numpy(), up.numpy()
        assert not bool((x.unsqueeze(-1) == lut).any()), "x == q: the reference's CPU index there is undefined"
        for kind, fn in (("identity", Q.nns), ("poly", Q.nns_poly), ("sigmoid", Q.nns_sigmoid)):
            for tag, s in S.items():
                xa = x.clone().requires_grad_(True)
                q = fn(xa, torch.tensor(s, dtype=dt))
                q.backward(up)
                out[f"nns_grad_{kind}_{tag}_{p}"] = xa.grad.numpy()
                if f"nns_q_{p}" in out:
                    assert np.array_equal(out[f"nns_q_{p}"], q.detach().numpy())
                out[f"nns_q_{p}"] = q.detach().numpy()
        if dt == torch.float32:  # Quantization builds float32 scalars
            qz = Q.Quantization("nn_sigmoid", lut=[float(v) for v in tabs["n9"]], num_bits=3, dev=torch.device("cpu"))
            xa = x.clone().requires_grad_(True)
            o = qz(xa, ITER_FRAC)
            o.sum().backward()
            out[f"quant_sigmoid_{p}"], out[f"quant_sigmoid_grad_{p}"] = o.detach().numpy(), xa.grad.numpy()
        for n, xin in (("x4", x4), ("x6", x6)):
            xa = xin.to(dt).clone().requires_grad_(True)
            out[f"tv_{n}_{p}"] = xin.to(dt).numpy()
            tv = HF.total_variation(xa)
            tv.backward()
            out[f"tvval_{n}_{p}"] = tv.detach().numpy()
            out[f"tv_grad_{n}_{p}"] = xa.grad.numpy()
            x4d = xin.to(dt).reshape(-1, *xin.shape[-3:])
            dx, dy = HF.center_difference(x4d)
            out[f"cd_dx_{n}_{p}"], out[f"cd_dy_{n}_{p}"] = dx.numpy(), dy.numpy()
        out[f"snap_x_{p}"] = snap_x.to(dt).numpy()
        luts = {"1": torch.tensor([0, 1, 2, 3]) * (1 * MM / 4), "2": torch.tensor([0, 1, 2, 3, 4, 5, 6, 7]) * (1 * MM / 8),
                "3": torch.arange(0, 10) * (1 * MM / 10)}
        for k, lut in luts.items():  # the notebooks' formula, evaluated here (see the docstring)
            out[f"snap_lut_{k}"] = lut.double().numpy()
            lut = lut.to(dt)
            idx = torch.argmin(torch.abs(snap_x.to(dt).unsqueeze(-1) - lut), dim=-1)
            out[f"snap_idx_{k}_{p}"], out[f"snap_q_{k}_{p}"] = idx.numpy(), lut[idx].numpy()
    out["quant_iter_frac"] = np.float64(ITER_FRAC)
    D.lut = D.lut_midvals = None
    path = os.path.join(HERE, "heightmap_golden.npz")
    np.savez_compressed(path, **out)
    print("entries", len(out), "wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
