#!/usr/bin/env python
"""Time the far-field kernels (farfield.pattern_grid, orders, pattern) on the current GPU and write
profiles/farfield_timing.txt.

  fields [1, 8, 2048, 2048] and [1, 1, 1024, 1024] complex64; a 256 x 256 (u, v) grid, 7 x 7 orders, a 4096-direction cut
  (a) the hand kernels
  (b) the same algebra as torch.einsum on the materialised complex64 tables (farfield.axis_table) in two steps, with
      the intermediate in memory -- what a user writes without the kernel -- on the same card
  (c) for the cut also points.rs_points at r = 1e3 m (fewer rounds: it is an O(M H W) sum of transcendentals)

HIP events around each call, every shape warmed up, the contenders alternated round by round; medians and the spread
(min .. max).  Peak memory is torch's allocator peak above the resident field and tables.  FLOP/s are 8 R K N per pass
over the call's time.  No traffic counter is read.
"""
import argparse
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quantizationawarethzdoe_amd import farfield, points  # noqa: E402


def measure(fns, n):
    """the contenders alternated round by round -> per contender (milliseconds, peak bytes above the start)"""
    peaks = []
    for f in fns:
        for _ in range(2):
            f()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        f()
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - base)
    ms = [[] for _ in fns]
    for _ in range(n):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    return list(zip(ms, peaks))


def fmt(r, flop=None):
    v, peak = r
    med = statistics.median(v)
    rate = f" {flop / (med * 1e-3) / 1e12:6.2f} TFLOP/s" if flop else ""
    return f"{med:9.3f} ms ({min(v):.3f} .. {max(v):.3f}){rate} peak {peak / 2 ** 20:7.1f} MiB"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "farfield_timing.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pitch = 0.25e-3
    lines = [f"Far-field timing on {torch.cuda.get_device_name(0)}; {args.rounds} rounds, median (min .. max); "
             "FLOP/s on 8 R K N per pass; traffic counters not read", ""]
    for B, C, H, W in ((1, 8, 2048, 2048), (1, 1, 1024, 1024)):
        wl = [1e-3 * (1 + 0.05 * c) for c in range(C)]
        U = torch.randn(B, C, H, W, dtype=torch.complex64, device=dev)
        planes = B * C
        lines += [f"field {tuple(U.shape)} complex64 ({8.0 * U.numel() / 2 ** 20:.0f} MiB)"]

        def contest(name, hand, eins, flop, extra=()):
            err = float((hand() - eins()).norm() / eins().norm())
            r = measure([hand, eins], args.rounds)
            ratio = statistics.median(r[1][0]) / statistics.median(r[0][0])
            lines.append(f"  {name:<22s} hand {fmt(r[0], flop)}   einsum {fmt(r[1], flop)}   einsum / hand {ratio:5.2f}"
                         f"   rel diff {err:.1e}")
            for what, fn, n in extra:
                lines.append(f"  {'':<22s} {what} {fmt(measure([fn], n)[0])}")

        # a 256 x 256 (u, v) grid over +-30 degrees
        u, v = (a.to(dev) for a in farfield.uv_grid(math.radians(30), 256))
        Ex = farfield.axis_table(W, pitch, 0.0, u, wl, device=dev)
        Ey = farfield.axis_table(H, pitch, 0.0, v, wl, device=dev)
        contest("grid 256 x 256", lambda: farfield.pattern_grid(U, u, v, pitch, wl),
                lambda: torch.einsum("cvi,bciu->bcvu", Ey, torch.einsum("bcij,cuj->bciu", U, Ex)) * (pitch * pitch),
                8.0 * planes * (H * W * 256 + 256 * H * 256))
        # 7 x 7 orders of a period of 64 pixels
        ms = tuple(range(-3, 4))
        f = torch.tensor([m / (64 * pitch) for m in ms], dtype=torch.float64, device=dev)
        Fx = farfield.axis_table(W, pitch, 0.0, f, space="frequency", device=dev).expand(C, -1, -1)
        Fy = farfield.axis_table(H, pitch, 0.0, f, space="frequency", device=dev).expand(C, -1, -1)

        def orders_einsum():
            a = torch.einsum("cvi,bciu->bcvu", Fy, torch.einsum("bcij,cuj->bciu", U, Fx)) * (1.0 / (H * W))
            return a.real.square() + a.imag.square()

        contest("orders 7 x 7", lambda: farfield.orders(U, 64 * pitch, ms, ms, pitch), orders_einsum,
                8.0 * planes * (H * W * 7 + 7 * H * 7))
        # a 4096-direction cut in the phi = 30 degree plane
        dirs = farfield.cut(math.radians(30), torch.linspace(-1.2, 1.2, 4096, dtype=torch.float64)).to(dev)
        Cx = farfield.axis_table(W, pitch, 0.0, dirs[:, 0].contiguous(), wl, device=dev)
        Cy = farfield.axis_table(H, pitch, 0.0, dirs[:, 1].contiguous(), wl, device=dev)
        w = torch.sqrt(1 - (dirs ** 2).sum(-1))
        pts = 1e3 * torch.cat([dirs, w[:, None]], -1)
        contest("cut 4096", lambda: farfield.pattern(U, dirs, pitch, wl),
                lambda: (torch.einsum("bcij,cmj->bcim", U, Cx) * Cy.transpose(-1, -2)).sum(-2) * (pitch * pitch),
                8.0 * planes * H * W * 4096,
                [("points.rs_points at r = 1e3 m", lambda: points.rs_points(U, pts, wl, pitch), 3)])
        lines.append("")
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
