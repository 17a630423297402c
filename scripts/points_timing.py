#!/usr/bin/env python
"""Time the point-propagation kernels (points.rs_points, forward and forward + backward) on the current GPU and write
profiles/points_timing.txt.

A 1024^2 field at 0.5 mm pitch, C = 1 and C = 8, to 512 points of a scan line, to a 64 x 64 and to a 256 x 256 tilted
plane; and the C = 1 field to the 256^2 on-grid pixel centres of one plane against RSC_prop, which returns that whole
plane by FFT and is expected to win by a wide margin.

The yardstick is the same sum written with torch ops under the same contract (fp64 geometry and phase reduction, fp32
amplitude, a complex64 einsum), chunked over the points so that the kernel matrix of a chunk fits in memory; its forward
+ backward takes each chunk's backward at once, so no chunk's matrix is kept.  It is linear in the number of points by
construction, so above ``--torch-points`` points it is timed on that many and scaled, and the line says so.  HIP events
around each call, warmed up, the two contenders alternated round by round; medians and the spread, peak memory above the
inputs.  Kernel time is the library's own event pair around each launch (thz_timing_read) in a pass of its own.  No
counter is read.
"""
import argparse
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quantizationawarethzdoe_amd import _lib, points  # noqa: E402

DX = 0.5e-3


def torch_points(U, pts, lam, per_chunk, backward=False):
    """the sum with torch ops, ``per_chunk`` points at a time; ``backward``: also the gradient of sum |out|^2"""
    B, C, H, W = U.shape
    dev = U.device
    x = ((torch.arange(W, dtype=torch.float64, device=dev) - (W - 1) / 2) * DX).repeat(H)
    y = ((torch.arange(H, dtype=torch.float64, device=dev) - (H - 1) / 2) * DX).repeat_interleave(W)
    lam64 = torch.tensor(lam, dtype=torch.float64, device=dev)[:, None, None]
    Uf = U.detach().reshape(B, C, H * W).requires_grad_(backward)
    outs = []
    for m0 in range(0, pts.shape[0], per_chunk):
        p = pts[m0:m0 + per_chunk]
        z = p[:, 2, None]
        r = torch.sqrt((p[:, 0, None] - x) ** 2 + (p[:, 1, None] - y) ** 2 + z ** 2)
        t = r[None] / lam64
        ang = (2 * math.pi) * (t - torch.floor(t)).float()
        rf = r.float()
        amp = (z.float() / (2 * math.pi * rf ** 2) * (DX * DX))[None]
        G = torch.polar(torch.ones_like(ang), ang) * torch.complex((amp / rf).expand_as(ang), -(amp * (2 * math.pi / lam64).float()))
        out = torch.einsum("bcp,cmp->bcm", Uf, G)
        if backward:
            (out.real ** 2 + out.imag ** 2).sum().backward()
        outs.append(out.detach())
    return Uf.grad if backward else torch.cat(outs, -1)


def hand(U, pts, lam, backward=False):
    x = U.detach().requires_grad_(backward)
    out = points.rs_points(x, pts, wavelengths=lam, spacing=DX)
    if backward:
        (out.real ** 2 + out.imag ** 2).sum().backward()
        return x.grad
    return out


def rounds(fns, n):
    """the contenders alternated round by round -> per contender (milliseconds per round, peak bytes above the start)"""
    peaks = []
    for f in fns:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        f()
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
    return ms, peaks


def fmt(v, scale=1.0):
    return f"{scale * statistics.median(v):10.3f} ms ({scale * min(v):.3f} .. {scale * max(v):.3f})"


def kernel_ms(fn, names, calls=3):
    """per call, the event time of each named kernel family"""
    _lib.timing_enable(True)
    try:
        _lib.timing_reset()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return [_lib.timing_read(n)[0] / calls for n in names]
    finally:
        _lib.timing_enable(False)
        _lib.timing_reset()


class Lines(list):
    """the report's lines, printed as they come"""

    def append(self, line):
        print(line, flush=True)
        super().append(line)

    def __iadd__(self, more):
        for line in more:
            self.append(line)
        return self


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--torch-points", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points_timing.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N = args.size
    tilt = dict(center=(0.0, 0.0, 60e-3), tilt_y=math.radians(20))
    targets = [("scan line, 512 points", points.scan_line((-40e-3, 0, 50e-3), (40e-3, 0, 80e-3), 512)),
               ("tilted plane 64 x 64", points.tilted_plane((64, 64), 1e-3, **tilt).reshape(-1, 3)),
               ("tilted plane 256 x 256", points.tilted_plane((256, 256), 0.25e-3, **tilt).reshape(-1, 3))]
    lines = Lines()
    lines += [f"points timing on {torch.cuda.get_device_name(0)}; field {N}^2 at {DX * 1e3} mm; {args.rounds} rounds, median "
             "(min .. max); peak = peak memory above the inputs; a hand kernel that loses is marked **", ""]
    for C in (1, 8):
        lam = torch.linspace(0.8e-3, 1.5e-3, C).tolist() if C > 1 else [1e-3]
        U = torch.randn(1, C, N, N, dtype=torch.complex64, device=dev)
        per_chunk = max(1, 64 // C)
        for name, host in targets:
            pts = host.to(dev)
            M = pts.shape[0]
            sub = pts[:args.torch_points]
            scale = M / sub.shape[0]
            note = f" (timed on {sub.shape[0]} points, x{scale:.0f})" if scale > 1 else ""
            lines.append(f"C = {C}, {name}: {M * N * N * C / 1e9:.2f} G (pair, channel)")
            for what, bw in (("forward", False), ("forward + backward", True)):
                ms, peaks = rounds([lambda: hand(U, pts, lam, bw), lambda: torch_points(U, sub, lam, per_chunk, bw)],
                                   args.rounds if M <= 4096 else 3)
                h, t = statistics.median(ms[0]), scale * statistics.median(ms[1])
                lines.append(f"  {'**' if h > t else '  '}{what:<19s} hand {fmt(ms[0])} peak {peaks[0] / 2**20:7.1f} MiB | torch "
                             f"{fmt(ms[1], scale)} peak {peaks[1] / 2**20:7.0f} MiB{note}  x{t / h:6.1f}")
            k = kernel_ms(lambda: hand(U, pts, lam, True), ["rs_points_fwd", "rs_points_finish", "rs_points_adj"])
            rate = M * N * N * C / 1e9
            lines.append(f"    kernels: fwd {k[0]:.3f} ms ({rate / k[0]:.1f} T pair-channels/s), finish {k[1]:.3f} ms, "
                         f"adj {k[2]:.3f} ms ({rate / k[2]:.1f} T pair-channels/s)")
            lines.append("")
        if C == 1:
            from quantizationawarethzdoe_amd.DataType.ElectricField import ElectricField
            from quantizationawarethzdoe_amd.Props.RSC_Prop import RSC_prop
            field = ElectricField(U, wavelengths=lam, spacing=DX, device=dev)
            rsc = RSC_prop(z_distance=60e-3, device=dev)
            grid = points.tilted_plane((256, 256), DX, (0.0, 0.0, 60e-3)).reshape(-1, 3).to(dev)
            ms, peaks = rounds([lambda: hand(U, grid, lam), lambda: rsc(field).data], 3)
            h, t = statistics.median(ms[0]), statistics.median(ms[1])
            lines.append("C = 1, the 256^2 on-grid pixel centres of the plane z = 60 mm against RSC_prop (the whole plane by FFT)")
            lines.append(f"  {'**' if h > t else '  '}forward             hand {fmt(ms[0])} peak {peaks[0] / 2**20:7.1f} MiB | RSC_prop "
                         f"{fmt(ms[1])} peak {peaks[1] / 2**20:7.0f} MiB  x{t / h:6.3f}")
            lines.append("")
        del U
        torch.cuda.empty_cache()
    lines.append("Traffic counters: not read.  A rocprofv3 kernel trace was not made: kernel times are the library's launch events.")
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
