#!/usr/bin/env python
"""Time the Zernike kernels (zernike.project / synthesize / fit, ZernikeDOEElement) on the current GPU and write
profiles/zernike_timing.txt.

  shapes     2048^2 and 1024^2 maps, a pupil inscribed in the grid, K = 120 (n_max = 14) and K = 6 (n_max = 2),
             B = 1, 8 and 32
  baseline   the same algebra as torch.matmul on a materialised float32 table [K, H W] on the same card (the exported
             table of the kernels; building it is not timed), the fit with the same cached Cholesky factor
  memory     peak allocation above the inputs (and, for the baseline, above its table, which is reported separately)

HIP events around each call, every shape warmed up, the two contenders alternated round by round; medians and the
spread (min .. max).
The rates are the MFMA flops issued (whole 32-row tiles of K times 32 plane columns per pupil pixel, whatever B) and
the maps' bytes over the event time of the whole call (its finish
kernel and, for the fit, the solve included).  No traffic counter is read.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quantizationawarethzdoe_amd import doe, zernike  # noqa: E402
from quantizationawarethzdoe_amd.Components.ZernikeDOE import ZernikeDOEElement  # noqa: E402
from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField  # noqa: E402

DX, LAM, MATERIAL = 0.5e-3, 1e-3, [2.66, 0.03]


def rounds(fns, n):
    """the contenders alternated round by round -> per contender (list of milliseconds, peak bytes above the start)"""
    for f in fns:
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms, peak = [[] for _ in fns], [0 for _ in fns]
    for _ in range(n):
        for i, f in enumerate(fns):
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = f()
            b.record()
            b.synchronize()
            del out
            ms[i].append(a.elapsed_time(b))
            peak[i] = max(peak[i], torch.cuda.max_memory_allocated() - base)
    return ms, peak


def fmt(v):
    return f"{statistics.median(v):8.3f} ms ({min(v):.3f} .. {max(v):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zernike_timing.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"Zernike kernels on {torch.cuda.get_device_name(0)}; {args.rounds} rounds, median (min .. max); hand = the "
             "kernels, torch = matmul on a materialised [K, H W] float32 table; peak = allocation above the inputs", ""]
    for n_pix in (2048, 1024):
        pupil = (0.0, 0.0, (n_pix / 2 - 1) * DX)
        npup = zernike.pupil_pixels((n_pix, n_pix), DX, pupil)
        for n_max in (14, 2):
            K = zernike.num_modes(n_max)
            rows = 32 * -(-K // 32)           # the K rows the matrix cores multiply: whole 32-row tiles
            pairs = {1: 1, 2: 3, 3: 6, 4: 10}[rows // 32]  # Gram tile pairs computed
            T = zernike.zernike_table((n_pix, n_pix), DX, pupil, n_max, dev).reshape(K, -1)
            geo = zernike._geometry((n_pix, n_pix), DX, pupil, n_max, "timing")
            L = zernike._gram(geo, dev, "timing")[1]
            (mg,), _ = rounds([lambda: zernike._project(None, geo, dev, gram=True)], 5)
            tg = statistics.median(mg) * 1e-3
            lines.append(f"--- {n_pix}^2, K = {K}: {npup} pupil pixels; the baseline's table is {T.numel() * 4 / 2**20:.0f} MiB; "
                         f"the Gram matrix, once per pupil: {fmt(mg)}, {2.0 * pairs * 32 * 32 * npup / tg / 1e12:.2f} TFLOP/s on "
                         f"its {pairs} computed 32 x 32 tile(s)")
            for B in (1, 8, 32):
                w = torch.randn(B, n_pix, n_pix, device=dev)
                a = torch.randn(B, K, device=dev)
                ops = {
                    "project": (lambda: zernike.project(w, DX, pupil, n_max), lambda: w.view(B, -1) @ T.T,
                                2.0 * rows * 32 * -(-B // 32) * npup, 4.0 * B * npup),
                    "synthesize": (lambda: zernike.synthesize(a, (n_pix, n_pix), DX, pupil),
                                   lambda: (a @ T).view(B, n_pix, n_pix),
                                   2.0 * rows * 32 * -(-B // 32) * npup, 4.0 * B * n_pix * n_pix),
                    "fit": (lambda: zernike.fit(w, DX, pupil, n_max),
                            lambda: torch.cholesky_solve((w.view(B, -1) @ T.T).double().T, L).T.float(),
                            2.0 * rows * 32 * -(-B // 32) * npup, 4.0 * B * npup),
                }
                for name, (hand, base, flop, byts) in ops.items():
                    err = float((hand() - base()).norm() / base().norm())
                    (mh, mt), (ph, pt) = rounds([hand, base], args.rounds)
                    t = statistics.median(mh) * 1e-3
                    lines.append(f"{name:10s} B {B:2d}: hand {fmt(mh)} peak {ph / 2**20:7.1f} MiB   torch {fmt(mt)} peak "
                                 f"{pt / 2**20:7.1f} MiB   torch / hand {statistics.median(mt) / statistics.median(mh):6.2f}   "
                                 f"MFMA model {flop / t / 1e12:6.2f} TFLOP/s, maps {byts / t / 1e12:5.3f} TB/s   rel diff {err:.1e}")
            # the element: forward + backward to the coefficients, one plane
            U = torch.randn(1, 1, n_pix, n_pix, dtype=torch.complex64, device=dev)
            p = torch.nn.Parameter(1e-4 * torch.randn(K, device=dev))
            elem = ZernikeDOEElement(p, pupil, (n_pix, n_pix), DX, MATERIAL, device=dev)
            q = torch.nn.Parameter(p.detach().clone())

            def step_hand():
                p.grad = None
                f = ElectricField(U, wavelengths=LAM, spacing=[DX, DX], device=dev)
                elem(f).data.abs().pow(2).sum().backward()

            def step_torch():
                q.grad = None
                out, _ = doe.modulate(U, (q @ T).view(n_pix, n_pix), [LAM], *MATERIAL)
                out.abs().pow(2).sum().backward()

            (mh, mt), (ph, pt) = rounds([step_hand, step_torch], args.rounds)
            lines.append(f"element fwd + bwd: hand {fmt(mh)} peak {ph / 2**20:7.1f} MiB   torch {fmt(mt)} peak "
                         f"{pt / 2**20:7.1f} MiB   torch / hand {statistics.median(mt) / statistics.median(mh):6.2f}")
            del T
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
