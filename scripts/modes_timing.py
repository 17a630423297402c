#!/usr/bin/env python
"""Time the Hermite-Gauss decomposition (modes.hg_decompose, utils.metrics.gaussicity) on the current GPU and write
profiles/modes_timing.txt.

  field [3, 32, 2048, 2048] complex64 (--shape), 32 x 32 modes and 1 x 1
  (a) hg_decompose / gaussicity, forward and forward + backward (the gradient of sum |c|^2 to the field)
  (b) the same algebra as torch.einsum on the exported fp32 tables cast to complex64, in two steps with the
      [B, C, H, N] intermediate materialised -- what a user writes without the kernel -- on the same card
  (c) optics.region_stats on the same field: the project's existing read-the-field-once pass

HIP events around each call, every shape warmed up, the contenders alternated round by round; medians and the spread
(min .. max).  Peak memory is torch's allocator peak above the resident field.  The effective TB/s is the field's
8 bytes per pixel over the call's time; no traffic counter is read.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quantizationawarethzdoe_amd import modes, optics  # noqa: E402
from quantizationawarethzdoe_amd.utils import metrics  # noqa: E402


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


def fmt(r):
    v, peak = r
    return f"{statistics.median(v):8.3f} ms ({min(v):.3f} .. {max(v):.3f}) peak {peak / 2 ** 20:7.1f} MiB"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--shape", type=int, nargs=4, default=[3, 32, 2048, 2048])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "modes_timing.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, C, H, W = args.shape
    pitch, waist = 0.25e-3, [(0.1 + 0.001 * c) * W * 0.25e-3 for c in range(C)]
    U = torch.randn(B, C, H, W, dtype=torch.complex64, device=dev)
    byts = 8.0 * U.numel()
    lines = [f"Hermite-Gauss decomposition timing on {torch.cuda.get_device_name(0)}; field {tuple(U.shape)} complex64 "
             f"({byts / 2 ** 30:.2f} GiB); {args.rounds} rounds, median (min .. max)", ""]
    for M, N in ((32, 32), (1, 1)):
        Gx = modes.hg_table(N, W, pitch, waist, 0.0, dev).to(torch.complex64)
        Gy = modes.hg_table(M, H, pitch, waist, 0.0, dev).to(torch.complex64)

        def hand(x=U):
            return modes.hg_decompose(x, pitch, waist, orders=(M, N))

        def einsum(x=U):
            return torch.einsum("cmi,bcin->bcmn", Gy, torch.einsum("bcij,cnj->bcin", x, Gx)) * (pitch * pitch)

        def step(fn):
            def run():
                x = U.detach().requires_grad_(True)
                (fn(x).abs() ** 2).sum().backward()
                return x.grad
            return run

        err = float((hand() - einsum()).norm() / einsum().norm())
        fwd = measure([hand, einsum], args.rounds)
        bwd = measure([step(hand), step(einsum)], max(3, args.rounds // 2))
        t = statistics.median(fwd[0][0]) * 1e-3
        lines += [f"{M:2d} x {N:2d} modes, forward:            hand {fmt(fwd[0])}   einsum {fmt(fwd[1])}   einsum / hand "
                  f"{statistics.median(fwd[1][0]) / statistics.median(fwd[0][0]):5.2f}   rel diff {err:.1e}",
                  f"{M:2d} x {N:2d} modes, forward + backward: hand {fmt(bwd[0])}   einsum {fmt(bwd[1])}   einsum / hand "
                  f"{statistics.median(bwd[1][0]) / statistics.median(bwd[0][0]):5.2f}",
                  f"{M:2d} x {N:2d} modes, forward over the call: {byts / t / 1e12:5.2f} TB/s on 8 B per pixel"]
    g, r = measure([lambda: metrics.gaussicity(U, pitch, waist), lambda: optics.region_stats(U, [], "circ")], args.rounds)
    lines += ["", f"utils.metrics.gaussicity (hg_decompose 1 x 1 + region_stats): {fmt(g)}",
              f"optics.region_stats, whole plane, the same field:            {fmt(r)}   "
              f"{byts / (statistics.median(r[0]) * 1e-3) / 1e12:5.2f} TB/s"]
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
