"""Timing of the measurement kernels (optics.region_stats, optics.line_widths) against the torch op sequence of
tests/metrics_ref.py run on the same device.

region_stats forward and forward + backward on [3, 32, 2048, 2048] complex64 with K = 1, 9 (the nine spots of
qat.FOCI_MM scaled to the plane) and 16 regions; line_widths on [4096, 2048] float32.  Byte model (DESIGN.md
section 28): the forward reads 8 B per pixel and writes nothing of a plane's size; the backward reads 8 B and
writes 8 B per pixel; line_widths reads 4 B per sample.  Inputs rotate through more than the 256 MB last-level
cache: each field is 3.2 GB and two alternate; line_widths walks a ring of ten line sets of 33.6 MB.  So no call
finds its input cached.  Device events around `reps` calls after a warm-up; the median of `rounds` rounds.

    python scripts/metrics_timing.py [--out profiles/metrics_timing.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quantizationawarethzdoe_amd import optics, qat  # noqa: E402
from tests import metrics_ref as mr  # noqa: E402


def timed(fn, inputs, reps, rounds):
    for x in inputs:
        fn(x)
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for r in range(reps):
            fn(inputs[r % len(inputs)])
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return statistics.median(out), min(out), max(out)


def tables(H, W):
    one = [("circ", H / 2 + 0.3, W / 2 + 0.2, 0.06 * H, 0.0)]
    nine = [("circ", (a / 100 + 0.5) * (H - 1), (b / 100 + 0.5) * (W - 1), 0.03 * H, 0.0) for a, b in qat.FOCI_MM]
    sixteen = nine + [("rect", (0.1 + 0.12 * k) * H, (0.9 - 0.11 * k) * W, 0.02 * H, 0.04 * W) for k in range(7)]
    return {1: one, 9: nine, 16: sixteen}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_timing.txt"))
    ap.add_argument("--shape", type=int, nargs=4, default=[3, 32, 2048, 2048])
    ap.add_argument("--lines", type=int, nargs=2, default=[4096, 2048])
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_timing: needs the ROCm device; nothing is measured without it")
    dev = torch.device("cuda:0")
    B, C, H, W = args.shape
    g = torch.Generator(device=dev).manual_seed(0)
    fields = [torch.view_as_complex(torch.randn(B, C, H, W, 2, device=dev, generator=g)) for _ in range(2)]
    px = B * C * H * W
    log = [f"# {torch.cuda.get_device_name(0)}; field [{B}, {C}, {H}, {W}] complex64 = {8 * px / 1e6:.0f} MB, two "
           f"alternate (beyond the 256 MB last-level cache); median (min .. max) of {args.rounds} rounds of {args.reps} calls",
           "# byte model: forward 8 B / pixel read; forward + backward 24 B / pixel (8 + 8 read, 8 written); "
           "line_widths 4 B / sample", ""]
    for K, rows in tables(H, W).items():
        regions, kinds = [list(r[1:]) for r in rows], [r[0] for r in rows]

        def fwd(x):
            return optics.region_stats(x, regions, kinds)

        def fwd_bwd(x):
            x = x.detach().requires_grad_(True)
            st = optics.region_stats(x, regions, kinds)
            return torch.autograd.grad(st.power.sum() + st.moment1.sum() + st.moment2.sum(), x)

        def ref_fwd(x):
            with torch.no_grad():
                return [mr.region_sums(p, rows) for p in x.reshape(B, C, H, W)], mr.region_peaks(x.reshape(-1, H, W)[:C], rows)

        def ref_fwd_sums(x):  # the five sums only (no peak / argmax pass), plane batch by plane batch
            with torch.no_grad():
                return [mr.region_sums(p, rows) for p in x.reshape(B, C, H, W)]

        t = timed(fwd, fields, args.reps, args.rounds)
        log.append(f"region_stats forward        K = {K:2d}: {t[0]:8.3f} ms ({t[1]:.3f} .. {t[2]:.3f})  "
                   f"{8 * px / t[0] / 1e9:6.3f} TB/s")
        t2 = timed(fwd_bwd, fields, args.reps, args.rounds)
        log.append(f"region_stats fwd + bwd      K = {K:2d}: {t2[0]:8.3f} ms ({t2[1]:.3f} .. {t2[2]:.3f})  "
                   f"{24 * px / t2[0] / 1e9:6.3f} TB/s")
        tr = timed(ref_fwd_sums, fields, max(1, args.reps // 3), max(2, args.rounds // 2))
        log.append(f"torch sequence, five sums   K = {K:2d}: {tr[0]:8.3f} ms ({tr[1]:.3f} .. {tr[2]:.3f})  "
                   f"x{tr[0] / t[0]:.1f} the kernel's forward")
        print("\n".join(log[-3:]), flush=True)
    L, Wl = args.lines
    ring = [torch.rand(L, Wl, device=dev, generator=g) for _ in range(10)]
    t = timed(lambda v: optics.line_widths(v), ring, 20, args.rounds)
    log.append(f"line_widths [{L}, {Wl}] float32 (ring of {len(ring)} x {4 * L * Wl / 1e6:.1f} MB): {t[0]:8.3f} ms "
               f"({t[1]:.3f} .. {t[2]:.3f})  {4 * L * Wl / t[0] / 1e9:6.3f} TB/s")

    def ref_lines(v):  # peak, argmax and the two nearest crossings by masked index reductions
        pk, arg = v.max(dim=-1)
        below = v < 0.5 * pk[:, None]
        j = torch.arange(v.shape[-1], device=v.device)
        jl = torch.where(below & (j < arg[:, None]), j, -1).amax(dim=-1)
        jr = torch.where(below & (j > arg[:, None]), j, v.shape[-1]).amin(dim=-1)
        return pk, arg, jl, jr

    tr = timed(ref_lines, ring, 20, args.rounds)
    log.append(f"torch sequence (max, two masked index reductions; no interpolation): {tr[0]:8.3f} ms "
               f"({tr[1]:.3f} .. {tr[2]:.3f})  x{tr[0] / t[0]:.1f}")
    print("\n".join(log[-2:]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(log) + "\n")


if __name__ == "__main__":
    main()
